"""GPU: the RGB-domain distortion probe (dct3d_distortion_rgb_frames*) in the three colour modes of a
context -- planes, YCbCr, YCbCr + 4:2:0 -- at both depths.

Reference, independent of csrc/ and built on the package's integer definitions: the planes are the R, G, B planes,
rgb_to_ycbcr's or rgb_to_ycbcr420's; plane k decodes as quant_common.ref_frames(plane, tables[cand[k]], depth) (the
oracle's Java-semantics DCT around the numpy quantiser); the decoded planes go back through ycbcr_to_rgb /
ycbcr420_to_rgb; the squared difference against the source bytes is taken in integers, per cube of the frames' grid
over the pixels inside the frame.  Bits: quant_common.code_bits of the reference's quantised planes.  Every
comparison is an exact equality of integers.

Sizes, each the smallest at which one piece can go wrong: 16x16 (no edge anywhere, not even in the 4:2:0 chroma),
24x24 (luma aligned, chroma 12x12 has an edge), 17x9 (3x2 luma cubes over 2x1 chroma cubes: the clamped chroma fetch
in the last column and row), 61x45 (every edge, odd chroma 31x23), 5x3 (one cube, most lanes masked).  Two stacks:
the stack index of the decoded planes and of sse."""
import contextlib
import functools

import numpy as np
import pytest

import quant_common as qc
from conftest import ctx_option
from test_gpu_c420 import FOLD_SHAPE
from test_gpu_distortion import _table
from test_gpu_edge import _rare_content
from test_gpu_ycc import colour

pytestmark = pytest.mark.gpu

MODES = ("planes", "ycc", "c420")
SIZES = [(16, 16), (24, 24), (17, 9), (61, 45), (5, 3)]
STACKS = 2
T8 = ("ref", "q1", "q2", "q12", "ones", "all255", "seeded", "qt3")
T11 = T8 + ("qt7", "qt20", "qt64")
# name -> (table names, candidates [n][3] or None, ask for plane_sse and bits)
SETS = {
    "one": (("q2",), [(0, 0, 0)], False),
    "eight": (T8, [(i, (i + 3) % 8, (i + 5) % 8) for i in range(8)], True),       # all-different (Y, Cb, Cr)
    "eleven": (T11, [(i, (i + 4) % 11, (i + 7) % 11) for i in range(11)], False),  # more than one launch of each pass
    "repeat": (("q1", "q12", "seeded"), [(0, 1, 2), (2, 2, 0), (0, 1, 2)], False),
    "none": (("ref", "all255", "qt3"), None, True),
    "rare": (("q1", "ref"), [(0, 0, 0), (1, 0, 1)], True),
    "chk": (("all255", "q12"), [(0, 0, 0), (1, 1, 1), (0, 1, 0), (1, 0, 1)], True),
}


def _ctx(depth, gpu_ctx8, gpu_ctx4):
    return gpu_ctx8 if depth == 8 else gpu_ctx4


@contextlib.contextmanager
def mode_on(ctx, pkg, mode):
    ctx.set_option(pkg.DCT3D_OPT_COLOUR, pkg.DCT3D_COLOUR_PLANES if mode == "planes" else pkg.DCT3D_COLOUR_YCBCR)
    ctx.set_chroma(pkg.DCT3D_CHROMA_420 if mode == "c420" else pkg.DCT3D_CHROMA_444)
    try:
        yield ctx
    finally:
        ctx.set_chroma(pkg.DCT3D_CHROMA_444)
        ctx.set_option(pkg.DCT3D_OPT_COLOUR, pkg.DCT3D_COLOUR_PLANES)


@functools.lru_cache(maxsize=None)
def frames_of(content, depth, w, h, stacks):
    p = qc.pkg()
    if content == "rare":
        fr = _rare_content(p, depth, 3)
    elif content.startswith("cert"):  # "cert<H>@<y0>": rows y0 .. y0 + h of cert_common's colour content of H rows
        import cert_common as cc
        H, y0 = (int(v) for v in content[4:].split("@"))
        fr = cc.content("uniform", depth, 3, w, H, stacks)[:, y0:y0 + h]
    elif content.startswith("chk"):
        n = int(content[3:])
        z, y, x = np.ogrid[:stacks * depth, :h, :w]
        fr = np.repeat((255 * (((x // n) + (y // n) + (z // n)) & 1))[..., None], 3, axis=-1)
    else:
        fr = colour(content, depth, w, h, stacks)
    fr = np.ascontiguousarray(fr, np.uint8)
    assert fr.shape == (stacks * depth, h, w, 3)
    fr.setflags(write=False)
    return fr


@functools.lru_cache(maxsize=None)
def source_planes(content, depth, w, h, stacks, mode):
    p = qc.pkg()
    fr = frames_of(content, depth, w, h, stacks)
    if mode == "planes":
        pl = [fr[..., k] for k in range(3)]
    elif mode == "ycc":
        t = p.rgb_to_ycbcr(fr)
        pl = [t[..., k] for k in range(3)]
    else:
        pl = list(p.rgb_to_ycbcr420(fr))
    return tuple(np.ascontiguousarray(a) for a in pl)


@functools.lru_cache(maxsize=None)
def ref_plane(content, depth, w, h, stacks, mode, k, name):
    """plane k under table `name`: (the decoded plane, its squared error per stack, its bits per stack)"""
    pl = source_planes(content, depth, w, h, stacks, mode)[k]
    q, out = qc.ref_frames(pl, _table(depth, name), depth)
    sse = ((pl.astype(np.int64) - out.astype(np.int64)) ** 2).reshape(stacks, -1).sum(axis=1)
    bits = qc.code_bits(q).reshape(stacks, -1).sum(axis=1)
    out.setflags(write=False)
    return out, sse, bits


def ref_rgb(content, depth, w, h, stacks, mode, names, cand):
    """int64 [n_cand, stacks, C]: the candidates' squared errors per cube of the frames' grid"""
    p = qc.pkg()
    fr = frames_of(content, depth, w, h, stacks).astype(np.int64)
    wp, hp = p.padded_size(w, h)
    res = []
    for c in cand:
        dec = [ref_plane(content, depth, w, h, stacks, mode, k, names[c[k]])[0] for k in range(3)]
        if mode == "planes":
            y = np.stack(dec, axis=-1)
        elif mode == "ycc":
            y = p.ycbcr_to_rgb(np.stack(dec, axis=-1))
        else:
            y = p.ycbcr420_to_rgb(*dec)
        pad = np.zeros((stacks * depth, hp, wp), np.int64)
        pad[:, :h, :w] = ((fr - y.astype(np.int64)) ** 2).sum(axis=-1)
        res.append(pad.reshape(stacks, depth, hp // 8, 8, wp // 8, 8).sum(axis=(1, 3, 5)).reshape(stacks, -1))
    return np.stack(res)


def ref_planes(content, depth, w, h, stacks, mode, names, what):
    """int64 [T, stacks, 3]: what = 1 the planes' own squared errors, 2 their bits"""
    return np.stack([np.stack([ref_plane(content, depth, w, h, stacks, mode, k, n)[what] for k in range(3)], axis=-1)
                     for n in names])


def probe_dev(ctx, content, depth, w, h, stacks, names, cand, want, want_bits=None):
    """distortion_rgb_frames_dev with guard bands around d_cube_sse and the frames at the end of their allocation
    -> (sse, plane_sse or None, bits or None, cube sse [n_cand, stacks, C]).  want: the planes' errors and, unless
    want_bits says otherwise, the bits"""
    want_bits = want if want_bits is None else want_bits
    import torch
    p = qc.pkg()
    wp, hp = p.padded_size(w, h)
    C = (wp // 8) * (hp // 8)
    n_cand = len(names) if cand is None else len(cand)
    n = n_cand * stacks * C * 4
    buf, mid = qc.banded(torch, n, 0xA5)
    fr = frames_of(content, depth, w, h, stacks)
    store = torch.zeros(4096 + fr.size, dtype=torch.uint8, device="cuda")
    d_fr = store[4096:]
    d_fr.copy_(torch.from_numpy(np.array(fr)).reshape(-1))
    res = ctx.distortion_rgb_frames_dev(d_fr, w, h, stacks, [_table(depth, x) for x in names], cand, mid,
                                        want_planes=want, want_bits=want_bits)
    got, intact = qc.bands_intact(buf, n, 0xA5)
    assert intact, "a write outside d_cube_sse"
    assert np.array_equal(d_fr.cpu().numpy(), fr.reshape(-1)), "the frames were written"
    cubes = got.view(np.uint32).reshape(n_cand, stacks, C)
    if want and want_bits:
        return res + (cubes,)
    return (res[0], res[1], None, cubes) if want else (res[0], None, res[1], cubes) if want_bits else (res, None, None, cubes)


def check_case(ctx, pkg, content, depth, w, h, stacks, mode, set_name):
    names, cand, want = SETS[set_name]
    cl = [(i, i, i) for i in range(len(names))] if cand is None else cand
    with mode_on(ctx, pkg, mode):
        sse, plane_sse, bits, cubes = probe_dev(ctx, content, depth, w, h, stacks, names, cand, want)
        stats = ctx.stats()
        ref = ref_rgb(content, depth, w, h, stacks, mode, names, cl)
        print(f"{mode} {w}x{h}x{stacks} d{depth} {set_name}: sse {sse.tolist()} flagged {stats['n_flagged']}")
        assert np.array_equal(cubes.astype(np.int64), ref), f"{(cubes != ref).sum()} cubes differ from the reference"
        assert np.array_equal(sse.astype(np.int64), ref.sum(axis=-1)), "the per-stack sums differ from the reference"
        assert np.array_equal(sse.astype(np.int64), cubes.astype(np.int64).sum(axis=-1))
        if want:
            tabs = [_table(depth, x) for x in names]
            fr = frames_of(content, depth, w, h, stacks)
            assert np.array_equal(plane_sse.astype(np.int64), ref_planes(content, depth, w, h, stacks, mode, names, 1))
            assert np.array_equal(bits.astype(np.int64), ref_planes(content, depth, w, h, stacks, mode, names, 2))
            assert np.array_equal(bits, ctx.rate_frames(fr, tabs))
            if mode == "planes":
                d = ctx.distortion_frames(fr, tabs)
                assert np.array_equal(plane_sse, d)
                for i, c in enumerate(cl):
                    assert np.array_equal(sse[i], sum(d[c[k], :, k] for k in range(3)))
    return sse, cubes, stats


@pytest.mark.parametrize("set_name", ["eight"])
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("depth", [8, 4])
def test_every_size(pkg, gpu_ctx8, gpu_ctx4, depth, mode, w, h, set_name):
    """8 candidates of all-different (Y, Cb, Cr) indices, with the planes' errors and the bits, at every size"""
    check_case(_ctx(depth, gpu_ctx8, gpu_ctx4), pkg, "uniform", depth, w, h, STACKS, mode, set_name)


@pytest.mark.parametrize("set_name", ["one", "eleven", "repeat", "none"])
@pytest.mark.parametrize("w,h", [(61, 45), (17, 9)])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("depth", [8, 4])
def test_candidate_sets(pkg, gpu_ctx8, gpu_ctx4, depth, mode, w, h, set_name):
    """one candidate; 11 candidates over 11 tables (more than one launch of each pass); a repeated candidate;
    cand = None"""
    check_case(_ctx(depth, gpu_ctx8, gpu_ctx4), pkg, "ramp", depth, w, h, STACKS, mode, set_name)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("depth", [8, 4])
def test_equals_the_stream_calls(pkg, gpu_ctx8, gpu_ctx4, depth, mode):
    """the definition itself on the GPU: per candidate a constant-map encode_eg_frames_vqc + decode_eg_frames_vqc on
    a second context and a numpy squared difference give the host-pointer call's numbers"""
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    w, h = 61, 45
    names, cand, _ = SETS["eight"]
    tabs = [_table(depth, x) for x in names]
    fr = frames_of("uniform", depth, w, h, STACKS)
    with mode_on(ctx, pkg, mode):
        sse = ctx.distortion_rgb_frames(fr, tabs, cand)
    with pkg.Context(0, 8, 8, depth) as other, mode_on(other, pkg, mode):
        for i, c in enumerate(cand):
            m = np.tile(np.array(c, np.uint8), (STACKS, 1))
            out, _ = other.decode_eg_frames_vqc([b for b, _ in other.encode_eg_frames_vqc(fr, tabs, m)], w, h, STACKS, tabs, m)
            want = ((fr.astype(np.int64) - out.astype(np.int64)) ** 2).reshape(STACKS, -1).sum(axis=1)
            assert np.array_equal(sse[i].astype(np.int64), want), f"candidate {c}"


@pytest.mark.parametrize("mode", ["ycc", "c420"])
@pytest.mark.parametrize("depth", [8, 4])
def test_stack_ranges(pkg, gpu_ctx8, gpu_ctx4, depth, mode):
    """a call whose decoded planes exceed the plane budget (32 tables, every (table, plane) pair, 256 x 176), so that
    the stacks go in two ranges, the second of one stack (4:4:4: 1 + 1 stacks at 8 x 8 x 8, 3 + 1 at 8 x 8 x 4; 4:2:0:
    3 + 1 and 7 + 1): every number is the one the same call gives for each stack alone (one range), two candidates are the
    stream calls', and the first candidate's cubes are the numpy reference's"""
    import torch
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    w, h = 256, 176
    cw, ch = pkg.chroma_size(w, h) if mode == "c420" else (w, h)
    tabs = [pkg.quant_table(q, depth) for q in range(1, 33)]
    per_stack = len(tabs) * depth * (w * h + 2 * cw * ch)  # bytes of one stack's decoded planes
    stacks = pkg.DCT3D_RGB_PLANE_BUDGET // per_stack + 1     # one more than a range holds
    assert 2 <= stacks <= 8
    cand = [(i, (i + 5) % 32, (i + 11) % 32) for i in range(32)]
    fr = frames_of("uniform", depth, w, h, stacks)
    C = (w // 8) * (h // 8)
    with mode_on(ctx, pkg, mode):
        d_fr = torch.from_numpy(np.array(fr)).cuda()
        buf, mid = qc.banded(torch, 32 * stacks * C * 4, 0xA5)
        sse, planes, bits = ctx.distortion_rgb_frames_dev(d_fr, w, h, stacks, tabs, cand, mid, want_planes=True, want_bits=True)
        got, intact = qc.bands_intact(buf, 32 * stacks * C * 4, 0xA5)
        assert intact
        cubes = got.view(np.uint32).reshape(32, stacks, C)
        assert np.array_equal(sse.astype(np.int64), cubes.astype(np.int64).sum(axis=-1))
        names = tuple(f"qt{q}" for q in range(1, 33))  # (_table's names of the same tables)
        assert all(np.array_equal(_table(depth, names[i]), tabs[i]) for i in cand[0])
        ref = ref_rgb("uniform", depth, w, h, stacks, mode, names, cand[:1])
        assert np.array_equal(cubes[:1].astype(np.int64), ref), f"{(cubes[:1] != ref).sum()} cubes differ from the reference"
        one = torch.zeros(32 * C, dtype=torch.int32, device="cuda")
        for s in range(stacks):
            a, b, c = ctx.distortion_rgb_frames_dev(d_fr[s * depth:(s + 1) * depth], w, h, 1, tabs, cand, one,
                                                    want_planes=True, want_bits=True)
            assert np.array_equal(a[:, 0], sse[:, s]) and np.array_equal(b[:, 0], planes[:, s]) and np.array_equal(c[:, 0], bits[:, s])
            assert np.array_equal(one.cpu().numpy().view(np.uint32).reshape(32, C), cubes[:, s]), f"stack {s}"
        host = ctx.distortion_rgb_frames(fr, tabs, cand, want_planes=True, want_bits=True)
        assert all(np.array_equal(x, y) for x, y in zip(host, (sse, planes, bits)))
        assert np.array_equal(bits, ctx.rate_frames(fr, tabs))
    with pkg.Context(0, 8, 8, depth) as other, mode_on(other, pkg, mode):
        for i in (0, 31):
            m = np.tile(np.array(cand[i], np.uint8), (stacks, 1))
            out, _ = other.decode_eg_frames_vqc([x for x, _ in other.encode_eg_frames_vqc(fr, tabs, m)], w, h, stacks, tabs, m)
            want = ((fr.astype(np.int64) - out.astype(np.int64)) ** 2).reshape(stacks, -1).sum(axis=1)
            assert np.array_equal(sse[i].astype(np.int64), want), f"candidate {cand[i]}"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("depth", [8, 4])
def test_decode_replay(pkg, gpu_ctx8, gpu_ctx4, depth, mode):
    """a widened decode margin sends nearly every lane of both passes through the decode's exact replay: the results
    are those at the default margin (and the reference's), n_flagged is larger"""
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    plain, cubes, st0 = check_case(ctx, pkg, "uniform", depth, 61, 45, STACKS, mode, "repeat")
    with ctx_option(ctx, pkg.DCT3D_OPT_DEC_MARGIN, 0.25):
        sse, cubes1, st1 = check_case(ctx, pkg, "uniform", depth, 61, 45, STACKS, mode, "repeat")
    assert np.array_equal(sse, plain) and np.array_equal(cubes1, cubes)
    assert st1["n_flagged"] >= st0["n_flagged"] + cubes[0].size, "nearly every cube must take the replay"
    assert st1["n_units"] == st0["n_units"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("depth", [8, 4])
def test_encode_rare_path(pkg, gpu_ctx8, gpu_ctx4, depth, mode):
    """content whose coefficients the fp32 certificate leaves open, under quant_table(1): the exact folds settle them
    and the results are the reference's.  Planes mode: test_gpu_edge's rare content (its R plane is the grey rare
    content).  YCbCr modes: the planes are other planes, so the content is test_gpu_c420's FOLD_SHAPE, at which the
    fold runs in all three planes."""
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    if mode == "planes":
        _, _, st = check_case(ctx, pkg, "rare", depth, 29, 7, 48, mode, "rare")
    else:
        w, h, stacks = FOLD_SHAPE
        _, _, st = check_case(ctx, pkg, "uniform", depth, w, h, stacks, mode, "rare")
    assert st["n_flagged"] > 0, "the content must leave coefficients to the exact fold"


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("depth", [8, 4])
def test_saturation_and_clamp(pkg, gpu_ctx8, gpu_ctx4, depth, mode, n):
    """0 / 255 checkerboards under all255 and q12: the saturation in the plane decode and the clamp of the inverse
    colour transform"""
    check_case(_ctx(depth, gpu_ctx8, gpu_ctx4), pkg, f"chk{n}", depth, 24, 16, 1, mode, "chk")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("depth", [8, 4])
def test_context_state(pkg, gpu_ctx8, gpu_ctx4, depth, mode):
    """the call leaves the quantiser, the colour option and the chroma mode as they were; tables = None is the
    context's table; queued between two encode_eg_frames_vqc calls on a framework stream (a map that differs by stack
    and channel) it changes neither stream; distortion_frames is still refused under the colour option"""
    import torch
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
            none = ctx.distortion_rgb_frames(fr)
            assert np.array_equal(none, ctx.distortion_rgb_frames(fr, [_table(depth, "q2")], [(0, 0, 0)]))
            assert np.array_equal(none.astype(np.int64),
                                  ref_rgb("uniform", depth, w, h, STACKS, mode, ("q2",), [(0, 0, 0)]).sum(axis=-1))
            ctx.distortion_rgb_frames(fr, tabs, cand, want_planes=True, want_bits=True)
            assert np.array_equal(ctx.quant(), before_q) and ctx.chroma() == before_c
            assert ctx.encode_eg_frames(fr) == before  # (the colour option too: the streams are the mode's)
            if mode != "planes":
                with pytest.raises(pkg.Dct3dError) as e:
                    ctx.distortion_frames(fr)
                assert e.value.code == pkg.DCT3D_EINVAL
            # the per-(stack, channel) calls around the probe: the streams of the same calls without it
            m = np.array([[0, 1, 2], [2, 0, 1]], np.uint8)
            alone = ctx.encode_eg_frames_vqc(fr, tabs, m)
            assert alone != ctx.encode_eg_frames_vqc(fr, tabs, m[::-1].copy())  # (the map matters to these streams)
            d_fr = torch.from_numpy(np.array(fr)).cuda()
            caps = [(len(b) + 64 + 3) // 4 * 4 for b, _ in alone]
            outs = [[torch.zeros(c, dtype=torch.uint8, device="cuda") for c in caps] for _ in range(2)]
            s = torch.cuda.Stream()
            torch.cuda.synchronize()
            ctx.set_stream(s.cuda_stream)
            with torch.cuda.stream(s):
                tb0 = ctx.encode_eg_frames_vqc_dev(d_fr, w, h, 3, STACKS, tabs, m, outs[0], caps)
                mid = ctx.distortion_rgb_frames_dev(d_fr, w, h, STACKS, tabs, cand)
                tb1 = ctx.encode_eg_frames_vqc_dev(d_fr, w, h, 3, STACKS, tabs, m, outs[1], caps)
                ctx.synchronize()
            for tb, o in ((tb0, outs[0]), (tb1, outs[1])):
                assert tb == [bits for _, bits in alone]
                for ch, (b, _) in enumerate(alone):
                    assert o[ch].cpu().numpy()[:len(b)].tobytes() == b
            assert np.array_equal(mid.astype(np.int64), ref_rgb("uniform", depth, w, h, STACKS, mode, names, cand).sum(axis=-1))
    finally:
        ctx.synchronize()
        ctx.set_stream(None)
        ctx.set_quant(None)


# ---- the codec's psnr_rgb= ----------------------------------------------------------------------------------------

SUFFIXES = (".red", ".green", ".blue")


def _cli(pkg, *args):
    import subprocess
    r = subprocess.run([pkg.CLI_PATH] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def _same_files(tmp_path, a, b):
    for sfx in SUFFIXES:
        x, y = (tmp_path / (a + sfx)).read_bytes(), (tmp_path / (b + sfx)).read_bytes()
        assert x == y and len(x) > 0, f"{a}{sfx} and {b}{sfx} differ"


def _codec_case(pkg, tmp_path, depth):
    from test_gpu_distortion import LADDER
    w, h, frames = 61, 45, 16
    fr = frames_of("ramp", depth, w, h, frames // depth)
    raw = tmp_path / "in.raw"
    fr.tofile(raw)
    return w, h, frames, fr, raw, [pkg.quant_table(q, depth) for q in LADDER], LADDER


def _mid_target(pkg, errs, n_samples):
    """a target between two of the ladder's PSNRs (not at a boundary)"""
    db = sorted(set(pkg.psnr_db(int(e), n_samples) for e in errs))
    lo, hi = db[len(db) // 2 - 1], db[len(db) // 2]
    assert hi - lo > 1e-3
    return f"{(lo + hi) / 2:.4f}"


@pytest.mark.parametrize("depth", [8, 4])
def test_codec_psnr_rgb_ycc(pkg, gpu_ctx8, gpu_ctx4, tmp_path, depth):
    """encode_rgb psnr_rgb=<dB> ycc=1: the printed q is pick_quality_psnr's over the probe's ladder, the files are
    those of the explicit q=<n> ycc=1, and the printed PSNR is the one computed from the decoded file"""
    import re
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    w, h, frames, fr, raw, tabs, ladder = _codec_case(pkg, tmp_path, depth)
    with mode_on(ctx, pkg, "ycc"):
        sse, bits = ctx.distortion_rgb_frames(fr, tabs, want_bits=True)
    errs = sse.astype(object).sum(axis=1)
    T = _mid_target(pkg, errs, fr.size)
    want = pkg.pick_quality_psnr({q: int(e) for q, e in zip(ladder, errs)}, fr.size, float(T))
    out = _cli(pkg, "encode_rgb", raw, tmp_path / "p", w, h, frames, 1, depth, f"psnr_rgb={T}", "ycc=1")
    m = re.search(r"^psnr_rgb: q=(\d+),(\d+),(\d+) psnr=(\S+) bits=(\d+)$", out, re.M)
    assert m, out
    n = int(m.group(1))
    assert n == want and m.group(2) == m.group(3) == m.group(1)
    assert int(m.group(5)) == int(bits[ladder.index(n)].astype(object).sum())
    _cli(pkg, "encode_rgb", raw, tmp_path / "q", w, h, frames, 1, depth, f"q={n}", "ycc=1")
    _same_files(tmp_path, "p", "q")
    _cli(pkg, "decode_rgb", tmp_path / "p", tmp_path / "back.raw", w, h, frames, 1, depth, f"q={n}", "ycc=1")
    back = np.fromfile(tmp_path / "back.raw", np.uint8).reshape(fr.shape)
    err = int(((fr.astype(np.int64) - back.astype(np.int64)) ** 2).sum())
    assert m.group(4) == f"{pkg.psnr_db(err, fr.size):.3f}"


@pytest.mark.parametrize("depth", [8, 4])
def test_codec_psnr_rgb_c420_qmap3(pkg, gpu_ctx8, gpu_ctx4, tmp_path, depth):
    """encode_rgb psnr_rgb=<dB> ycc=1 chroma=420 qmap3=MAP cq=1: the written map is pick_stack_channel_qualities_psnr's
    on the probe's numbers, the files are those of the rerun that reads the map, and every stack of the decoded file
    reaches the PSNR the rule promised"""
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    w, h, frames, fr, raw, tabs, ladder = _codec_case(pkg, tmp_path, depth)
    T16 = len(ladder)
    cand = [(i, min(i + 1, T16 - 1), min(i + 1, T16 - 1)) for i in range(T16)]
    with mode_on(ctx, pkg, "c420"):
        sse = ctx.distortion_rgb_frames(fr, tabs, cand)
    per_stack = fr.size // (frames // depth)
    T = _mid_target(pkg, sse[:, 0], per_stack)
    want = pkg.pick_stack_channel_qualities_psnr(sse, ladder, per_stack, float(T), 1)
    tokens = ("ycc=1", "chroma=420", f"qmap3={tmp_path / 'map.txt'}")
    out = _cli(pkg, "encode_rgb", raw, tmp_path / "p", w, h, frames, 1, depth, f"psnr_rgb={T}", *tokens, "cq=1")
    assert "qmap3: stacks=%d bits=" % (frames // depth) in out, out
    got = [tuple(int(x) for x in line.split()) for line in (tmp_path / "map.txt").read_text().splitlines()]
    assert got == want
    _cli(pkg, "encode_rgb", raw, tmp_path / "q", w, h, frames, 1, depth, *tokens)
    _same_files(tmp_path, "p", "q")
    _cli(pkg, "decode_rgb", tmp_path / "p", tmp_path / "back.raw", w, h, frames, 1, depth, *tokens)
    back = np.fromfile(tmp_path / "back.raw", np.uint8).reshape(fr.shape)
    err = ((fr.astype(np.int64) - back.astype(np.int64)) ** 2).reshape(frames // depth, -1).sum(axis=1)
    for s, (q, _, _) in enumerate(want):
        assert int(err[s]) == int(sse[ladder.index(q), s]), f"stack {s}"


@pytest.mark.parametrize("depth", [8, 4])
def test_codec_psnr_rgb_planes_is_psnr(pkg, tmp_path, depth):
    """with ycc=0 psnr_rgb=<dB> prints the q, PSNR and bits of psnr=<dB> and writes the same files; so with qmap="""
    import re
    w, h, frames, fr, raw, tabs, ladder = _codec_case(pkg, tmp_path, depth)
    a = _cli(pkg, "encode_rgb", raw, tmp_path / "a", w, h, frames, 1, depth, "psnr=33.5")
    b = _cli(pkg, "encode_rgb", raw, tmp_path / "b", w, h, frames, 1, depth, "psnr_rgb=33.5")
    ma = re.search(r"^psnr: q=(\d+) psnr=(\S+) bits=(\d+)$", a, re.M)
    mb = re.search(r"^psnr_rgb: q=(\d+),(\d+),(\d+) psnr=(\S+) bits=(\d+)$", b, re.M)
    assert ma and mb, a + b
    assert (mb.group(1), mb.group(4), mb.group(5)) == ma.groups() and mb.group(2) == mb.group(3) == mb.group(1)
    _same_files(tmp_path, "a", "b")
    _cli(pkg, "encode_rgb", raw, tmp_path / "c", w, h, frames, 1, depth, "psnr=33.5", f"qmap={tmp_path / 'c.txt'}")
    _cli(pkg, "encode_rgb", raw, tmp_path / "d", w, h, frames, 1, depth, "psnr_rgb=33.5", f"qmap={tmp_path / 'd.txt'}")
    assert (tmp_path / "c.txt").read_text() == (tmp_path / "d.txt").read_text() != ""
    _same_files(tmp_path, "c", "d")
