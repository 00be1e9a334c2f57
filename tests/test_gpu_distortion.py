"""GPU: the distortion probe (dct3d_distortion_frames*) -- the exact squared error of encode + decode
under several quantiser tables from one transform -- and the codec's psnr= argument built on it.

The reference is independent of csrc/: quant_common.ref_frames (the oracle's Java-semantics DCT and inverse with
the numpy quantiser around them) gives the cubes and the cropped decode; the squared error is an int64 sum of
(frames - decoded)^2 per cube over the samples inside the frame, and per (stack, channel); quant_common.code_bits
gives the bits."""
import functools
import re
import subprocess

import numpy as np
import pytest

import quant_common as qc
from conftest import ctx_option
from test_gpu_edge import _rare_content

pytestmark = pytest.mark.gpu

LADDER = (1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 24, 32, 40, 48, 64)

# name -> (width, height, channels, stacks)
GEOMS = {
    "g64x64": (64, 64, 1, 2),
    "g61x45": (61, 45, 1, 3),  # ragged both ways: padded samples coded, not counted
    "rgb61x45": (61, 45, 3, 3),
    "g8x8": (8, 8, 1, 3),      # one cube per stack
    "g24x24": (24, 24, 1, 2),  # 9 cubes per stack: a wave straddles the stacks, the last wave is ragged
    "g5x3": (5, 3, 1, 1),      # w < 8
    "rare": (29, 7, 1, 48),
    "rare_rgb": (29, 7, 3, 48),
    "chk1": (24, 16, 1, 1),    # 0 / 255 checkerboards of 1, 2 and 4 pixel squares
    "chk2": (24, 16, 1, 1),
    "chk4": (21, 13, 1, 1),
}
MAIN_GEOMS = ["g64x64", "g61x45", "rgb61x45", "g8x8", "g24x24", "g5x3"]


def _ctx(depth, gpu_ctx8, gpu_ctx4):
    return gpu_ctx8 if depth == 8 else gpu_ctx4


@functools.lru_cache(maxsize=None)
def _frames(depth, geom):
    p = qc.pkg()
    w, h, channels, stacks = GEOMS[geom]
    if geom.startswith("rare"):
        fr = _rare_content(p, depth, channels)
    elif geom.startswith("chk"):
        n = int(geom[3:])
        z, y, x = np.ogrid[:stacks * depth, :h, :w]
        fr = (255 * (((x // n) + (y // n) + (z // n)) & 1)).astype(np.uint8)
    else:
        planes = [p.synthetic.frames(w, h, stacks * depth, seed=0x5EED + 17 * ch, frame0=3 + ch,
                                     kind="uniform" if ch != 1 else "ramp") for ch in range(channels)]
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


def cube_sums(sq, depth):
    """(frames - decoded)^2 [F, h, w] or [F, h, w, 3] (int64) -> [stacks, channels, cubes per stack and channel]: each
    cube of the padded raster sums its samples inside the frame"""
    if sq.ndim == 3:
        sq = sq[..., None]
    F, h, w, ch = sq.shape
    wp, hp = qc.pkg().padded_size(w, h)
    pad = np.zeros((F, hp, wp, ch), np.int64)
    pad[:, :h, :w] = sq
    c = pad.reshape(F // depth, depth, hp // 8, 8, wp // 8, 8, ch).sum(axis=(1, 3, 5))  # [stack, by, bx, ch]
    return np.ascontiguousarray(c.transpose(0, 3, 1, 2)).reshape(F // depth, ch, -1)


@functools.lru_cache(maxsize=None)
def _ref_case(depth, geom, name):
    """(squared error, bits) of every cube under the table, int64 [stacks, channels, C] each"""
    w, h, channels, stacks = GEOMS[geom]
    fr = _frames(depth, geom)
    q, out = qc.ref_frames(fr, _table(depth, name), depth)
    sse = cube_sums((fr.astype(np.int64) - out.astype(np.int64)) ** 2, depth)
    bits = qc.code_bits(q).reshape(q.shape[0], -1).sum(axis=1).reshape(stacks, channels, -1)
    assert sse.shape == bits.shape
    sse.setflags(write=False)
    bits.setflags(write=False)
    return sse, bits


def _ref(depth, geom, names, what=0):
    return np.stack([_ref_case(depth, geom, n)[what] for n in names])


def _probe_dev(ctx, depth, geom, names, want_bits=False):
    """distortion_frames_dev with a guarded cube map -> (sse [T, stacks, channels] or the pair with the bits,
    cube sse [T, stacks, channels, C])"""
    import torch
    w, h, channels, stacks = GEOMS[geom]
    wp, hp = qc.pkg().padded_size(w, h)
    C = (wp // 8) * (hp // 8)
    n = len(names) * stacks * channels * C * 4
    buf, mid = qc.banded(torch, n, 0xA5)
    d_fr = torch.from_numpy(np.array(_frames(depth, geom))).cuda()
    res = ctx.distortion_frames_dev(d_fr, w, h, channels, stacks, [_table(depth, x) for x in names], mid, want_bits)
    got, intact = qc.bands_intact(buf, n, 0xA5)
    assert intact, "a write outside d_cube_sse"
    return res, got.view(np.uint32).reshape(len(names), stacks, channels, C)


def _assert_equal_to_reference(sse, cubes, ref, names):
    for t, name in enumerate(names):
        assert np.array_equal(cubes[t].astype(np.int64), ref[t]), \
            f"table {name}: {(cubes[t] != ref[t]).sum()} cubes differ from the reference"
        assert np.array_equal(sse[t].astype(np.int64), ref[t].sum(axis=-1)), f"table {name}: the per-stack sums differ"


@pytest.mark.parametrize("n_tables", [1, 8, 11])
@pytest.mark.parametrize("geom", MAIN_GEOMS)
@pytest.mark.parametrize("depth", [8, 4])
def test_sse_equals_the_reference(gpu_ctx8, gpu_ctx4, depth, geom, n_tables):
    """1: per stack and channel, and per cube, the probe's squared error is the reference's, for 1, 8 and 11 (two
    launches) tables; nothing is written outside the cube map; the host call gives the same numbers."""
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    names = TABLE_SETS[n_tables]
    sse, cubes = _probe_dev(ctx, depth, geom, names)
    _assert_equal_to_reference(sse, cubes, _ref(depth, geom, names), names)
    assert ctx.stats()["n_units"] == cubes[0].size * 64 * depth * n_tables
    host = ctx.distortion_frames(_frames(depth, geom), [_table(depth, x) for x in names])
    assert np.array_equal(host, sse)


@pytest.mark.parametrize("geom", MAIN_GEOMS)
@pytest.mark.parametrize("depth", [8, 4])
def test_bits_equal_the_rate_probe(gpu_ctx8, gpu_ctx4, depth, geom):
    """2: the optional bits are rate_frames' for the same arguments (and the reference's); asking for them leaves
    the squared error as it is."""
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    names = TABLE_SETS[11]
    tabs = [_table(depth, x) for x in names]
    fr = _frames(depth, geom)
    (sse, bits), cubes = _probe_dev(ctx, depth, geom, names, want_bits=True)
    assert np.array_equal(bits, ctx.rate_frames(fr, tabs))
    assert np.array_equal(bits.astype(np.int64), _ref(depth, geom, names, 1).sum(axis=-1))
    _assert_equal_to_reference(sse, cubes, _ref(depth, geom, names), names)
    assert np.array_equal(ctx.distortion_frames(fr, tabs), sse)
    hs, hb = ctx.distortion_frames(fr, tabs, want_bits=True)
    assert np.array_equal(hs, sse) and np.array_equal(hb, bits)


@pytest.mark.parametrize("depth", [8, 4])
def test_host_call_in_several_chunks(gpu_ctx8, gpu_ctx4, depth):
    """1b: 40 frames of 1920 x 1080 (79 MiB) go up in two chunks of whole stacks on the host-pointer path: every
    (table, stack) sum lands at its place (the device call's numbers), and the chunks' statistics add up."""
    import torch
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    w, h, stacks = 1920, 1080, 40 // depth
    fr = np.random.default_rng(20261020).integers(0, 256, (40, h, w), dtype=np.uint8)
    fr[8:16] //= 4  # stacks that differ in what they cost
    tabs = [_table(depth, "q2"), _table(depth, "q12")]
    sse, bits = ctx.distortion_frames_dev(torch.from_numpy(fr).cuda(), w, h, 1, stacks, tabs, want_bits=True)
    units = ctx.stats()["n_units"]
    hs, hb = ctx.distortion_frames(fr, tabs, want_bits=True)
    assert ctx.stats()["n_units"] == units == 2 * fr.size
    assert np.array_equal(hs, sse) and np.array_equal(hb, bits)
    assert len(set(int(v) for v in sse[0, :, 0])) == stacks  # no two stacks alike: a misplaced chunk would show


def _unclamped(q, steps, depth):
    """the orthonormal inverse DCT of the dequantised cubes in plain fp64 (numpy), no clamp: [n, depth, 8, 8]"""
    def basis(N):
        k, n = np.ogrid[:N, :N]
        b = np.sqrt(2.0 / N) * np.cos((2 * n + 1) * k * np.pi / (2 * N))
        b[0] /= np.sqrt(2.0)
        return b
    c = np.asarray(q, np.float64).reshape(-1, depth, 8, 8) * qc.step_cube(steps, depth)
    return np.einsum("nabc,az,by,cx->nzyx", c, basis(depth), basis(8), basis(8))


@pytest.mark.parametrize("geom", ["chk1", "chk2", "chk4"])
@pytest.mark.parametrize("depth", [8, 4])
def test_clamp_and_truncation(depth, geom, gpu_ctx8, gpu_ctx4):
    """3: 0 / 255 checkerboards under coarse steps: decoded values leave [0, 255] by more than 1 (asserted on a plain
    numpy inverse of the reference's cubes, which the clamp has not touched), and the probe still equals the
    reference."""
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    names = ("all255", "q12")
    fr = _frames(depth, geom)
    for name in names:
        v = _unclamped(qc.ref_frames(fr, _table(depth, name), depth)[0], _table(depth, name), depth)
        assert ((v < -1.0) | (v > 256.0)).sum() > 0, f"table {name}: the content must have samples the decode clamps"
    sse, cubes = _probe_dev(ctx, depth, geom, names)
    _assert_equal_to_reference(sse, cubes, _ref(depth, geom, names), names)


@pytest.mark.parametrize("geom", ["rare", "rare_rgb"])
@pytest.mark.parametrize("depth", [8, 4])
def test_encode_rare_path(gpu_ctx8, gpu_ctx4, depth, geom):
    """4: content whose coefficients the fp32 certificate leaves open: the exact folds settle them (n_flagged > 0)
    and the squared error and the bits are still the reference's."""
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    (sse, bits), cubes = _probe_dev(ctx, depth, geom, RARE_TABLES, want_bits=True)
    flagged = ctx.stats()["n_flagged"]
    _assert_equal_to_reference(sse, cubes, _ref(depth, geom, RARE_TABLES), RARE_TABLES)
    assert np.array_equal(bits.astype(np.int64), _ref(depth, geom, RARE_TABLES, 1).sum(axis=-1))
    assert flagged > 0, "the content must leave coefficients to the exact fold"


@pytest.mark.parametrize("geom", ["rgb61x45", "g24x24"])
@pytest.mark.parametrize("depth", [8, 4])
def test_decode_rare_path(pkg, gpu_ctx8, gpu_ctx4, depth, geom):
    """5: a widened decode margin sends nearly every lane through the decode's exact replay, which reads the
    quantised values back from the wave's int16 copy: the sums are those at the default margin and the reference's."""
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    names = ("ref", "q1", "all255")
    plain, plain_cubes = _probe_dev(ctx, depth, geom, names)
    with ctx_option(ctx, pkg.DCT3D_OPT_DEC_MARGIN, 0.25):
        sse, cubes = _probe_dev(ctx, depth, geom, names)
        flagged = ctx.stats()["n_flagged"]
    assert flagged >= cubes[0].size, "nearly every cube must take the replay"
    assert np.array_equal(sse, plain) and np.array_equal(cubes, plain_cubes)
    _assert_equal_to_reference(sse, cubes, _ref(depth, geom, names), names)
    again, _ = _probe_dev(ctx, depth, geom, names)  # the option is restored
    assert np.array_equal(again, plain)


@pytest.mark.parametrize("depth", [8, 4])
def test_agrees_with_the_product_calls(pkg, gpu_ctx8, gpu_ctx4, depth):
    """6: for two tables, set_quant + encode_frames + decode_frames on a second context and a numpy sum of squares
    give the probe's numbers."""
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    geom = "rgb61x45"
    w, h, channels, stacks = GEOMS[geom]
    fr = _frames(depth, geom)
    names = ("q2", "seeded")
    sse = ctx.distortion_frames(fr, [_table(depth, x) for x in names])
    with pkg.Context(0, 8, 8, depth) as other:
        for t, name in enumerate(names):
            other.set_quant(_table(depth, name))
            out = other.decode_frames(other.encode_frames(fr), w, h, stacks, channels)
            want = cube_sums((fr.astype(np.int64) - out.astype(np.int64)) ** 2, depth).sum(axis=-1)
            assert np.array_equal(sse[t].astype(np.int64), want), f"table {name}"


@pytest.mark.parametrize("depth", [8, 4])
def test_context_state(gpu_ctx8, gpu_ctx4, depth):
    """7: a probe call leaves the context as it was: the quantiser, the next encode's bytes; tables=None is the
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
        none = ctx.distortion_frames(fr)
        assert np.array_equal(ctx.quant(), before_q)
        assert np.array_equal(none, ctx.distortion_frames(fr, [_table(depth, "q2")]))
        assert np.array_equal(none[0].astype(np.int64), _ref_case(depth, geom, "q2")[0].sum(axis=-1))
        ctx.distortion_frames(fr, others)
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
            mid = ctx.distortion_frames_dev(d_fr, w, h, channels, stacks, others)
            tb1 = ctx.encode_eg_frames_dev(d_fr, w, h, channels, stacks, outs[1], caps)
            ctx.synchronize()
        for tb, o in ((tb0, outs[0]), (tb1, outs[1])):
            assert tb == [bits for _, bits in before]
            for ch, (b, _) in enumerate(before):
                assert o[ch].cpu().numpy()[:len(b)].tobytes() == b
        assert np.array_equal(mid[0].astype(np.int64), _ref_case(depth, geom, "q1")[0].sum(axis=-1))
    finally:
        ctx.synchronize()
        ctx.set_stream(None)
        ctx.set_quant(None)


def _cli(pkg, *args):
    r = subprocess.run([pkg.CLI_PATH] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@pytest.mark.parametrize("target", ["mid", "high", "1"])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("depth", [8, 4])
def test_codec_psnr(pkg, tmp_path, depth, channels, target):
    """8: dct3d_codec encode / encode_rgb with psnr=: the printed q=<n> is pick_quality_psnr's over the reference's
    ladder (a target between two of the reference's ladder PSNRs, so not at a boundary), the files are those of the
    explicit q=<n>; a target above every ladder PSNR gives q=1, 1 dB gives q=64."""
    w, h, frames = 61, 45, 2 * depth
    planes = [pkg.synthetic.frames(w, h, frames, seed=0xC0DEC + ch, frame0=ch, kind="ramp" if ch else "uniform")
              for ch in range(channels)]
    fr = np.ascontiguousarray(planes[0] if channels == 1 else np.stack(planes, axis=-1), np.uint8)
    per_q, bits_q = {}, {}
    for q in LADDER:
        cubes, out = qc.ref_frames(fr, pkg.quant_table(q, depth), depth)
        per_q[q] = int(((fr.astype(np.int64) - out.astype(np.int64)) ** 2).sum())
        bits_q[q] = int(qc.code_bits(cubes).sum())
    n_samples = fr.size
    db = sorted(set(pkg.psnr_db(e, n_samples) for e in per_q.values()))
    assert len(db) >= 2 and np.isfinite(db[-1])
    if target == "mid":
        lo, hi = db[len(db) // 2 - 1], db[len(db) // 2]
        assert hi - lo > 1e-3
        T = f"{(lo + hi) / 2:.4f}"
    elif target == "high":
        T = f"{db[-1] + 5.0:.4f}"
    else:
        T = "1"
    want = pkg.pick_quality_psnr(per_q, n_samples, float(T))
    if target == "high":
        assert want == 1
    if target == "1":
        assert want == 64

    raw = tmp_path / "in.raw"
    fr.tofile(raw)
    enc = "encode" if channels == 1 else "encode_rgb"
    suffixes = [""] if channels == 1 else [".red", ".green", ".blue"]
    out = _cli(pkg, enc, raw, tmp_path / "p.bin", w, h, frames, 1, depth, f"psnr={T}")
    m = re.search(r"^psnr: q=(\d+) psnr=(\S+) bits=(\d+)$", out, re.M)
    assert m, out
    n = int(m.group(1))
    assert n == want
    assert m.group(2) == f"{pkg.psnr_db(per_q[n], n_samples):.3f}"
    _cli(pkg, enc, raw, tmp_path / "q.bin", w, h, frames, 1, depth, f"q={n}")
    assert int(m.group(3)) == bits_q[n]
    for sfx in suffixes:
        a, b = (tmp_path / ("p.bin" + sfx)).read_bytes(), (tmp_path / ("q.bin" + sfx)).read_bytes()
        assert a == b and len(a) > 0, f"psnr={T} and q={n} wrote different files{sfx}"
