"""GPU: the SSIM probe (dct3d_ssim_frames*) -- the exact 8 x 8 / stride 4 windowed SSIM of encode + decode
under several quantiser tables from one transform -- and the codec's ssim= argument built on it.

The reference is independent of csrc/: quant_common.ref_frames (the oracle's Java-semantics DCT and inverse with the
numpy quantiser around them) gives the decoded frames, ssim_windows_ref (the definition in numpy) the v of every
window; the per-(stack, channel) numbers are their int64 sums."""
import ctypes as C
import functools
import re
import subprocess

import numpy as np
import pytest

import quant_common as qc
from cert_common import MARGINS
from conftest import ctx_option
from test_gpu_edge import _rare_content

pytestmark = pytest.mark.gpu

LADDER = (1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 24, 32, 40, 48, 64)
ONE = 1 << 24
BAND = 4096

# name -> (width, height, channels, stacks)
GEOMS = {
    "g64x64": (64, 64, 1, 2),
    "rgb64x64": (64, 64, 3, 2),
    "g61x45": (61, 45, 1, 3),  # ragged both ways: windows of fewer than 64 samples at the right and bottom edges
    "rgb61x45": (61, 45, 3, 2),
    "g8x8": (8, 8, 1, 3),      # one cube and one window per frame
    "g24x24": (24, 24, 1, 2),  # 9 cubes per stack: a wave straddles the stacks; windows across the cube faces
    "g5x3": (5, 3, 1, 2),      # two blocks, one window of 15 samples
    "g4x4": (4, 4, 1, 2),      # one block
    "g9x4": (9, 4, 1, 2),      # three block columns, the last of one sample column; one block row
    "g1x1": (1, 1, 1, 2),
    "rare": (29, 7, 1, 48),
    "rare_rgb": (29, 7, 3, 48),
    "chk1": (24, 16, 1, 1),    # 0 / 255 checkerboards of 1, 2 and 4 pixel squares
    "chk2": (24, 16, 1, 1),
    "chk4": (21, 13, 1, 1),
    "ranges": (256, 176, 1, 0),  # the stack count follows from the budget
}
MAIN_GEOMS = ["g64x64", "rgb64x64", "g61x45", "rgb61x45", "g8x8", "g24x24", "g5x3", "g4x4", "g9x4", "g1x1"]


def _ctx(depth, gpu_ctx8, gpu_ctx4):
    return gpu_ctx8 if depth == 8 else gpu_ctx4


def _range_stacks(depth):
    per_stack = depth * (256 // 4) * (176 // 4) * (8 * 32 + 4)
    return qc.pkg().DCT3D_SSIM_BLOCK_BUDGET // per_stack + 1


@functools.lru_cache(maxsize=None)
def _frames(depth, geom):
    """noise and ramp: the stacks (and the channels) alternate between the two"""
    p = qc.pkg()
    w, h, channels, stacks = GEOMS[geom]
    if geom == "ranges":
        stacks = _range_stacks(depth)
    if geom.startswith("rare"):
        fr = _rare_content(p, depth, channels)
    elif geom.startswith("chk"):
        n = int(geom[3:])
        z, y, x = np.ogrid[:stacks * depth, :h, :w]
        fr = (255 * (((x // n) + (y // n) + (z // n)) & 1)).astype(np.uint8)
    else:
        planes = []
        for ch in range(channels):
            kinds = [p.synthetic.frames(w, h, stacks * depth, seed=0x551A + 17 * ch, frame0=3 + ch, kind=k)
                     for k in ("uniform", "ramp")]
            pl = np.empty_like(kinds[0])
            for s in range(stacks):
                pl[s * depth:(s + 1) * depth] = kinds[(s + ch) & 1][s * depth:(s + 1) * depth]
            planes.append(pl)
        fr = planes[0] if channels == 1 else np.stack(planes, axis=-1)
    fr = np.ascontiguousarray(fr, np.uint8)
    fr.setflags(write=False)
    return fr


@functools.lru_cache(maxsize=None)
def _table(depth, name):
    p = qc.pkg()
    if name == "ref":
        t = p.quant_table(5, depth)
    elif name.startswith("qt"):
        t = p.quant_table(int(name[2:]), depth)
    else:
        t = qc.tables(depth)[name]
    t = np.array(t, np.int32)
    t.setflags(write=False)
    return t


TABLES8 = ("ref", "q1", "q2", "q12", "ones", "all255", "seeded", "qt3")
TABLE_SETS = {1: ("ref",), 8: TABLES8, 11: TABLES8 + ("qt7", "qt20", "qt64")}
RARE_TABLES = ("ref", "q1", "q12", "seeded")


def windows_of(fr, out, depth):
    """frames and decoded frames [F, h, w] or [F, h, w, 3] -> int64 [stacks, channels, depth, nwy, nwx]"""
    p = qc.pkg()
    if fr.ndim == 3:
        fr, out = fr[..., None], out[..., None]
    F = fr.shape[0]
    v = np.stack([p.ssim_windows_ref(np.ascontiguousarray(fr[..., ch]), np.ascontiguousarray(out[..., ch]))
                  for ch in range(fr.shape[-1])], axis=1)  # [F, ch, nwy, nwx]
    v = v.reshape(F // depth, depth, *v.shape[1:]).transpose(0, 2, 1, 3, 4)
    return np.ascontiguousarray(v)


@functools.lru_cache(maxsize=None)
def _ref_case(depth, geom, name):
    fr = _frames(depth, geom)
    _, out = qc.ref_frames(fr, _table(depth, name), depth)
    v = windows_of(fr, out, depth)
    v.setflags(write=False)
    return v


def _ref(depth, geom, names):
    return np.stack([_ref_case(depth, geom, n) for n in names])


def _probe_dev(ctx, depth, geom, names, **kw):
    """ssim_frames_dev with a guarded window map -> (the call's result, the windows [T, stacks, channels, D, nwy, nwx])"""
    import torch
    fr = _frames(depth, geom)
    w, h, channels = GEOMS[geom][:3]
    stacks = fr.shape[0] // depth
    nwx, nwy = qc.pkg().ssim_windows(w, h)
    shape = (len(names), stacks, channels, depth, nwy, nwx)
    n = int(np.prod(shape)) * 4
    buf, mid = qc.banded(torch, n, 0xA5)
    d_fr = torch.from_numpy(np.array(fr)).cuda()
    res = ctx.ssim_frames_dev(d_fr, w, h, channels, stacks, [_table(depth, x) for x in names], mid, **kw)
    got, intact = qc.bands_intact(buf, n, 0xA5)
    assert intact, "a write outside d_window_ssim"
    return res, got.view(np.int32).reshape(shape)


def _host_banded(ctx, fr, tabs, depth):
    """dct3d_ssim_frames itself with 4 KiB bands around its three host outputs -> (ssim, sse, bits)"""
    p = qc.pkg()
    channels = 1 if fr.ndim == 3 else 3
    stacks, h, w = fr.shape[0] // depth, fr.shape[1], fr.shape[2]
    tb = np.ascontiguousarray(np.stack(tabs), np.int32)
    n = len(tabs) * stacks * channels * 8
    bufs = [np.full(BAND + n + BAND, 0x5A, np.uint8) for _ in range(3)]
    ptr = [b.ctypes.data + BAND for b in bufs]
    fr = np.ascontiguousarray(fr)
    rc = p.lib().dct3d_ssim_frames(ctx._h, fr.ctypes.data, w, h, channels, stacks, tb.ctypes.data, len(tabs),
                                   C.c_void_p(ptr[0]), C.c_void_p(ptr[1]), C.c_void_p(ptr[2]))
    assert rc == p.DCT3D_OK
    for b in bufs:
        assert (b[:BAND] == 0x5A).all() and (b[BAND + n:] == 0x5A).all(), "a write outside the host call's outputs"
    shape = (len(tabs), stacks, channels)
    return (bufs[0][BAND:BAND + n].view(np.int64).reshape(shape), bufs[1][BAND:BAND + n].view(np.uint64).reshape(shape),
            bufs[2][BAND:BAND + n].view(np.uint64).reshape(shape))


def _assert_equal_to_reference(ssim, wins, ref, names):
    for t, name in enumerate(names):
        assert np.array_equal(wins[t].astype(np.int64), ref[t]), \
            f"table {name}: {(wins[t] != ref[t]).sum()} of {ref[t].size} windows differ from the reference"
        assert np.array_equal(ssim[t], ref[t].sum(axis=(-3, -2, -1))), f"table {name}: the per-stack sums differ"


@pytest.mark.parametrize("n_tables", [1, 8, 11])
@pytest.mark.parametrize("geom", MAIN_GEOMS)
@pytest.mark.parametrize("depth", [8, 4])
def test_ssim_equals_the_reference(gpu_ctx8, gpu_ctx4, depth, geom, n_tables):
    """1: every window's v and the per-(stack, channel) sums are the reference's, for 1, 8 and 11 (two launches) tables;
    nothing is written outside the window map or the host call's outputs; the host call gives the same numbers; sse
    and bits are distortion_frames'."""
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    names = TABLE_SETS[n_tables]
    tabs = [_table(depth, x) for x in names]
    fr = _frames(depth, geom)
    ssim, wins = _probe_dev(ctx, depth, geom, names)
    assert ssim.dtype == np.int64
    _assert_equal_to_reference(ssim, wins, _ref(depth, geom, names), names)
    wp, hp = qc.pkg().padded_size(*GEOMS[geom][:2])
    assert ctx.stats()["n_units"] == ssim[0].size * (wp // 8) * (hp // 8) * 64 * depth * n_tables
    hs, he, hb = _host_banded(ctx, fr, tabs, depth)
    assert np.array_equal(hs, ssim)
    sse, bits = ctx.distortion_frames(fr, tabs, want_bits=True)
    assert np.array_equal(he, sse) and np.array_equal(hb, bits)
    assert np.array_equal(ctx.ssim_frames(fr, tabs), ssim)


@pytest.mark.parametrize("geom", ["rgb61x45", "g24x24", "g5x3"])
@pytest.mark.parametrize("depth", [8, 4])
def test_sse_and_bits_equal_the_distortion_probe(gpu_ctx8, gpu_ctx4, depth, geom):
    """2: want_sse and want_bits, each alone and together, on the device and the host call: exactly
    distortion_frames(..., want_bits=True); asking for them leaves the SSIM as it is."""
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    names = TABLE_SETS[11]
    tabs = [_table(depth, x) for x in names]
    fr = _frames(depth, geom)
    sse, bits = ctx.distortion_frames(fr, tabs, want_bits=True)
    plain, _ = _probe_dev(ctx, depth, geom, names)
    (s1, e1), _ = _probe_dev(ctx, depth, geom, names, want_sse=True)
    (s2, b2), _ = _probe_dev(ctx, depth, geom, names, want_bits=True)
    (s3, e3, b3), wins = _probe_dev(ctx, depth, geom, names, want_sse=True, want_bits=True)
    for s in (s1, s2, s3):
        assert np.array_equal(s, plain)
    assert np.array_equal(e1, sse) and np.array_equal(e3, sse) and np.array_equal(b2, bits) and np.array_equal(b3, bits)
    _assert_equal_to_reference(s3, wins, _ref(depth, geom, names), names)
    hs, he, hb = ctx.ssim_frames(fr, tabs, want_sse=True, want_bits=True)
    assert np.array_equal(hs, plain) and np.array_equal(he, sse) and np.array_equal(hb, bits)
    hs, hb = ctx.ssim_frames(fr, tabs, want_bits=True)
    assert np.array_equal(hs, plain) and np.array_equal(hb, bits)


@pytest.mark.parametrize("geom", ["chk1", "chk2", "chk4"])
@pytest.mark.parametrize("depth", [8, 4])
def test_saturating_checkerboards(depth, geom, gpu_ctx8, gpu_ctx4):
    """3: 0 / 255 checkerboards under an all-255 table and quant_table(12): the decode saturates, the moments are at
    their largest, and the windows are still the reference's."""
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    names = ("all255", "q12")
    ssim, wins = _probe_dev(ctx, depth, geom, names)
    ref = _ref(depth, geom, names)
    _assert_equal_to_reference(ssim, wins, ref, names)
    assert (ref < ONE).any()


@pytest.mark.parametrize("geom", ["rare", "rare_rgb"])
@pytest.mark.parametrize("depth", [8, 4])
def test_encode_rare_path(gpu_ctx8, gpu_ctx4, depth, geom):
    """4: content whose coefficients the fp32 certificate leaves open: the exact folds settle them (n_flagged > 0) and
    the windows, the squared error and the bits are still right."""
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    (ssim, sse, bits), wins = _probe_dev(ctx, depth, geom, RARE_TABLES, want_sse=True, want_bits=True)
    flagged = ctx.stats()["n_flagged"]
    _assert_equal_to_reference(ssim, wins, _ref(depth, geom, RARE_TABLES), RARE_TABLES)
    es, eb = ctx.distortion_frames(_frames(depth, geom), [_table(depth, x) for x in RARE_TABLES], want_bits=True)
    assert np.array_equal(sse, es) and np.array_equal(bits, eb)
    assert flagged > 0, "the content must leave coefficients to the exact fold"


@pytest.mark.parametrize("geom", ["rgb61x45", "g24x24"])
@pytest.mark.parametrize("depth", [8, 4])
def test_decode_rare_path(pkg, gpu_ctx8, gpu_ctx4, depth, geom):
    """5: a widened decode margin sends nearly every lane through the decode's exact replay: the numbers are those at the
    default margin and the reference's."""
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    names = ("ref", "q1", "all255")
    plain, plain_wins = _probe_dev(ctx, depth, geom, names)
    with ctx_option(ctx, pkg.DCT3D_OPT_DEC_MARGIN, 0.25):
        ssim, wins = _probe_dev(ctx, depth, geom, names)
        flagged = ctx.stats()["n_flagged"]
    wp, hp = pkg.padded_size(*GEOMS[geom][:2])
    assert flagged >= ssim[0].size * (wp // 8) * (hp // 8), "nearly every cube must take the replay"
    assert np.array_equal(ssim, plain) and np.array_equal(wins, plain_wins)
    _assert_equal_to_reference(ssim, wins, _ref(depth, geom, names), names)
    again, _ = _probe_dev(ctx, depth, geom, names)  # the option is restored
    assert np.array_equal(again, plain)


@pytest.mark.parametrize("depth", [8, 4])
def test_ranges_of_stacks(pkg, gpu_ctx8, gpu_ctx4, depth):
    """6: 32 tables at 256 x 176 and one stack more than the block budget holds: the call walks the stacks in two
    ranges.  Every number equals the same call on each stack alone; the first table's windows are the reference's."""
    import torch
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    stacks = _range_stacks(depth)
    assert 2 <= stacks <= 8
    w, h = GEOMS["ranges"][:2]
    fr = _frames(depth, "ranges")
    assert fr.shape[0] == stacks * depth
    tabs = [pkg.quant_table(q, depth) for q in range(1, 33)]
    (ssim, sse, bits), wins = _probe_dev(ctx, depth, "ranges", [f"qt{q}" for q in range(1, 33)], want_sse=True, want_bits=True)
    assert len(set(int(v) for v in ssim[0, :, 0])) == stacks  # no two stacks alike: a misplaced range would show
    nwx, nwy = pkg.ssim_windows(w, h)
    for s in range(stacks):
        one = torch.from_numpy(np.array(fr[s * depth:(s + 1) * depth])).cuda()
        d_win = torch.zeros((32, 1, 1, depth, nwy, nwx), dtype=torch.int32, device="cuda")
        s1, e1, b1 = ctx.ssim_frames_dev(one, w, h, 1, 1, tabs, d_win, want_sse=True, want_bits=True)
        assert np.array_equal(s1[:, 0], ssim[:, s]) and np.array_equal(e1[:, 0], sse[:, s]) and np.array_equal(b1[:, 0], bits[:, s])
        assert np.array_equal(d_win.cpu().numpy()[:, 0], wins[:, s]), f"stack {s}"
    ref = _ref_case(depth, "ranges", "qt1")
    assert np.array_equal(wins[0].astype(np.int64), ref) and np.array_equal(ssim[0], ref.sum(axis=(-3, -2, -1)))


@pytest.mark.parametrize("depth", [8, 4])
def test_host_call_in_several_chunks(pkg, gpu_ctx8, gpu_ctx4, depth):
    """7: 40 frames of 1920 x 1080 (79 MiB) go up in two chunks of whole stacks on the host-pointer path: every (table,
    stack) sum lands at its place (the device call's numbers), and the chunks' statistics add up.  At MARGINS[0], where
    open coefficients and replayed lanes both count, the host call's n_flagged is the device call's and
    distortion_frames_dev's on the same raster (which test_gpu_probe_certificates.py holds to the emulation at this
    size): no chunk's or range's launches clear the slot the ones before counted into."""
    import torch
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    w, h, stacks = 1920, 1080, 40 // depth
    fr = np.random.default_rng(20261021).integers(0, 256, (40, h, w), dtype=np.uint8)
    fr[8:16] //= 4  # stacks that differ in what they cost
    tabs = [_table(depth, "q2"), _table(depth, "q12")]
    ssim, sse, bits = ctx.ssim_frames_dev(torch.from_numpy(fr).cuda(), w, h, 1, stacks, tabs, want_sse=True, want_bits=True)
    units = ctx.stats()["n_units"]
    hs, he, hb = ctx.ssim_frames(fr, tabs, want_sse=True, want_bits=True)
    assert ctx.stats()["n_units"] == units == 2 * fr.size
    assert np.array_equal(hs, ssim) and np.array_equal(he, sse) and np.array_equal(hb, bits)
    assert len(set(int(v) for v in ssim[0, :, 0])) == stacks  # no two stacks alike: a misplaced chunk would show
    with ctx_option(ctx, pkg.DCT3D_OPT_DEC_MARGIN, MARGINS[0]):
        d_fr = torch.from_numpy(fr).cuda()
        ds = ctx.ssim_frames_dev(d_fr, w, h, 1, stacks, tabs)
        dev = ctx.stats()
        hs = ctx.ssim_frames(fr, tabs)
        host = ctx.stats()
        de = ctx.distortion_frames_dev(d_fr, w, h, 1, stacks, tabs)
        dist = ctx.stats()
    assert np.array_equal(ds, ssim) and np.array_equal(hs, ssim) and np.array_equal(de, sse)
    print(f"8x8x{depth} margin {MARGINS[0]}: n_flagged device {dev['n_flagged']}, host {host['n_flagged']}, distortion {dist['n_flagged']}")
    assert host["n_units"] == dev["n_units"] == dist["n_units"] == units
    assert host["n_flagged"] == dev["n_flagged"] == dist["n_flagged"] > 32 * stacks  # replays in every stack, and open coefficients


@pytest.mark.parametrize("depth", [8, 4])
def test_context_state(gpu_ctx8, gpu_ctx4, depth):
    """8: a probe call leaves the context as it was: the quantiser, the next encode's bytes; tables=None is the
    context's table; queued between two encodes on a framework stream it changes neither."""
    import torch
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    geom = "rgb61x45"
    w, h, channels, stacks = GEOMS[geom]
    fr = _frames(depth, geom)
    others = [_table(depth, x) for x in ("q1", "all255", "seeded")]
    try:
        ctx.set_quant(_table(depth, "q2"))
        before_q = ctx.quant()
        before = ctx.encode_eg_frames(fr)
        none = ctx.ssim_frames(fr)
        assert np.array_equal(ctx.quant(), before_q)
        assert np.array_equal(none, ctx.ssim_frames(fr, [_table(depth, "q2")]))
        assert np.array_equal(none[0], _ref_case(depth, geom, "q2").sum(axis=(-3, -2, -1)))
        ctx.ssim_frames(fr, others)
        assert np.array_equal(ctx.quant(), before_q)
        assert ctx.encode_eg_frames(fr) == before
        # queued on a framework stream between two encodes
        d_fr = torch.from_numpy(np.array(fr)).cuda()
        caps = [(len(b) + 64 + 3) // 4 * 4 for b, _ in before]
        outs = [[torch.zeros(c, dtype=torch.uint8, device="cuda") for c in caps] for _ in range(2)]
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        ctx.set_stream(s.cuda_stream)
        with torch.cuda.stream(s):
            tb0 = ctx.encode_eg_frames_dev(d_fr, w, h, channels, stacks, outs[0], caps)
            mid = ctx.ssim_frames_dev(d_fr, w, h, channels, stacks, others)
            tb1 = ctx.encode_eg_frames_dev(d_fr, w, h, channels, stacks, outs[1], caps)
            ctx.synchronize()
        for tb, o in ((tb0, outs[0]), (tb1, outs[1])):
            assert tb == [bits for _, bits in before]
            for ch, (b, _) in enumerate(before):
                assert o[ch].cpu().numpy()[:len(b)].tobytes() == b
        assert np.array_equal(mid[0], _ref_case(depth, geom, "q1").sum(axis=(-3, -2, -1)))
    finally:
        ctx.synchronize()
        ctx.set_stream(None)
        ctx.set_quant(None)


@pytest.mark.parametrize("depth", [8, 4])
def test_refused_in_the_ycbcr_modes(pkg, gpu_ctx8, gpu_ctx4, depth):
    """9: packed RGB24 frames on a context whose colour transform or 4:2:0 mode is on: DCT3D_EINVAL from both calls;
    back in planes mode the call works again."""
    import torch
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    geom = "rgb61x45"
    w, h, channels, stacks = GEOMS[geom]
    fr = _frames(depth, geom)
    d_fr = torch.from_numpy(np.array(fr)).cuda()
    plain = ctx.ssim_frames(fr)
    calls = (lambda: ctx.ssim_frames(fr), lambda: ctx.ssim_frames_dev(d_fr, w, h, channels, stacks))
    try:
        # 4:2:0 set on a planes-mode context: refused for packed RGB24 by the chroma mode alone; grey frames have no
        # chroma and are measured as ever
        ctx.set_chroma(pkg.DCT3D_CHROMA_420)
        for call in calls:
            with pytest.raises(pkg.Dct3dError) as e:
                call()
            assert e.value.code == pkg.DCT3D_EINVAL
        grey = np.ascontiguousarray(fr[..., 0])
        assert np.array_equal(ctx.ssim_frames(grey)[:, :, 0], plain[:, :, 0])
        ctx.set_chroma(pkg.DCT3D_CHROMA_444)
        with ctx_option(ctx, pkg.DCT3D_OPT_COLOUR, pkg.DCT3D_COLOUR_YCBCR):
            for chroma in (pkg.DCT3D_CHROMA_444, pkg.DCT3D_CHROMA_420):
                ctx.set_chroma(chroma)
                for call in calls:
                    with pytest.raises(pkg.Dct3dError) as e:
                        call()
                    assert e.value.code == pkg.DCT3D_EINVAL
    finally:
        ctx.set_chroma(pkg.DCT3D_CHROMA_444)
    assert np.array_equal(ctx.ssim_frames(fr), plain)


def _cli(pkg, *args):
    r = subprocess.run([pkg.CLI_PATH] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@functools.lru_cache(maxsize=None)
def _codec_case(depth, channels):
    """frames of 61 x 45 (2 stacks) and, per ladder quality, the reference's per-stack sums of v [stacks] and bits"""
    p = qc.pkg()
    w, h, frames = 61, 45, 2 * depth
    planes = [p.synthetic.frames(w, h, frames, seed=0xC0DEC + ch, frame0=ch, kind="ramp" if ch else "uniform")
              for ch in range(channels)]
    fr = np.ascontiguousarray(planes[0] if channels == 1 else np.stack(planes, axis=-1), np.uint8)
    fr[depth:] //= 3  # the second stack is cheaper to code well
    per_q, bits_q = {}, {}
    for q in LADDER:
        cubes, out = qc.ref_frames(fr, p.quant_table(q, depth), depth)
        per_q[q] = windows_of(fr, out, depth).sum(axis=(-3, -2, -1))  # [stacks, channels]
        bits_q[q] = int(qc.code_bits(cubes).sum())
    return fr, per_q, bits_q


@pytest.mark.parametrize("target", ["mid", "high", "low"])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("depth", [8, 4])
def test_codec_ssim(pkg, tmp_path, depth, channels, target):
    """10: dct3d_codec encode / encode_rgb with ssim=: the printed q=<n> is pick_quality_ssim's over the reference's
    ladder (a target between two of the ladder's means, so not at a boundary), the printed mean is Python's to its six
    decimals, the files are those of the explicit q=<n>; a target of 1 gives q=1 unless a quality is lossless, a tiny
    target q=64."""
    w, h, frames = 61, 45, 2 * depth
    fr, per_q, bits_q = _codec_case(depth, channels)
    nwx, nwy = pkg.ssim_windows(w, h)
    n_windows = nwx * nwy * frames * channels
    tot = {q: int(v.sum()) for q, v in per_q.items()}
    means = sorted(set(pkg.ssim_mean(t, n_windows) for t in tot.values()))
    assert len(means) >= 2
    if target == "mid":
        lo, hi = means[len(means) // 2 - 1], means[len(means) // 2]
        assert hi - lo > 1e-5
        T = f"{(lo + hi) / 2:.6f}"
    elif target == "high":
        T = "1"
    else:
        T = "0.000001"
    want = pkg.pick_quality_ssim(tot, n_windows, float(T))
    if target == "high":
        assert means[-1] < 1.0 and want == 1
    if target == "low":
        assert means[0] > 1e-6 and want == 64

    raw = tmp_path / "in.raw"
    fr.tofile(raw)
    enc = "encode" if channels == 1 else "encode_rgb"
    suffixes = [""] if channels == 1 else [".red", ".green", ".blue"]
    out = _cli(pkg, enc, raw, tmp_path / "p.bin", w, h, frames, 1, depth, f"ssim={T}")
    m = re.search(r"^ssim: q=(\d+) ssim=(\S+) bits=(\d+)$", out, re.M)
    assert m, out
    n = int(m.group(1))
    assert n == want
    assert m.group(2) == f"{pkg.ssim_mean(tot[n], n_windows):.6f}"
    _cli(pkg, enc, raw, tmp_path / "q.bin", w, h, frames, 1, depth, f"q={n}")
    assert int(m.group(3)) == bits_q[n]
    for sfx in suffixes:
        a, b = (tmp_path / ("p.bin" + sfx)).read_bytes(), (tmp_path / ("q.bin" + sfx)).read_bytes()
        assert a == b and len(a) > 0, f"ssim={T} and q={n} wrote different files{sfx}"


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("depth", [8, 4])
def test_codec_ssim_qmap(pkg, tmp_path, depth, channels):
    """11: ssim=<t> qmap=<path> writes the map pick_stack_qualities_ssim gives on the reference's numbers, and the map
    round-trips: an encode with qmap=<path> alone writes the same files, a decode with it gives the frames the
    reference decodes stack by stack."""
    w, h, frames = 61, 45, 2 * depth
    fr, per_q, _ = _codec_case(depth, channels)
    nwx, nwy = pkg.ssim_windows(w, h)
    per_stack = nwx * nwy * depth * channels
    ssim = np.stack([per_q[q] for q in LADDER])  # [T, stacks, channels]
    means = sorted(set(pkg.ssim_mean(int(ssim[t, s].sum()), per_stack) for t in range(len(LADDER)) for s in range(2)))
    k = len(means) // 2
    assert means[k] - means[k - 1] > 1e-5
    T = f"{(means[k - 1] + means[k]) / 2:.6f}"
    want = pkg.pick_stack_qualities_ssim(ssim, LADDER, per_stack, float(T))
    assert len(set(want)) == 2, "the two stacks must get different qualities"

    raw = tmp_path / "in.raw"
    fr.tofile(raw)
    enc, dec = ("encode", "decode") if channels == 1 else ("encode_rgb", "decode_rgb")
    suffixes = [""] if channels == 1 else [".red", ".green", ".blue"]
    qmap = tmp_path / "map.txt"
    out = _cli(pkg, enc, raw, tmp_path / "p.bin", w, h, frames, 1, depth, f"ssim={T}", f"qmap={qmap}")
    assert re.search(r"^qmap: stacks=2 bits=\d+$", out, re.M), out
    assert [int(x) for x in qmap.read_text().split()] == want
    _cli(pkg, enc, raw, tmp_path / "m.bin", w, h, frames, 1, depth, f"qmap={qmap}")
    for sfx in suffixes:
        a, b = (tmp_path / ("p.bin" + sfx)).read_bytes(), (tmp_path / ("m.bin" + sfx)).read_bytes()
        assert a == b and len(a) > 0, sfx
    _cli(pkg, dec, tmp_path / "p.bin", tmp_path / "back.raw", w, h, frames, 1, depth, f"qmap={qmap}")
    back = np.fromfile(tmp_path / "back.raw", np.uint8).reshape(fr.shape)
    for s, q in enumerate(want):
        _, ref = qc.ref_frames(fr[s * depth:(s + 1) * depth], pkg.quant_table(q, depth), depth)
        assert np.array_equal(back[s * depth:(s + 1) * depth], ref), f"stack {s}"
