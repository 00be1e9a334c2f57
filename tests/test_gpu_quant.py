"""GPU: quantiser tables (dct3d_ctx_set_quant) through every raster call family, bit-exact against the
reference of quant_common.py -- the oracle's Java DCT around the numpy definition of the quantiser.

Shapes as test_gpu_geometry_sweep.py counts them: 8x8 (1 cube per stack), 24x16 (6), 40x24 (15), 136x72 (153), and
the ragged 13x9 and 50x21; 1 and 3 stacks; grey and packed RGB24 (the planar-stacked definition); both
depths.  Content: ramp, uniform noise and a 0 / 255 checkerboard (ties and saturation) -- a clip of 3 stacks holds
one stack of each, a clip of 1 stack takes them in turn over the cases.  The tables T: quant_common.tables."""
import functools
import os
import subprocess
import zlib

import numpy as np
import pytest

import quant_common as qc
from conftest import ctx_option
from test_gpu_eg import _expected

pytestmark = pytest.mark.gpu

SHAPES = [(8, 8), (24, 16), (40, 24), (136, 72), (13, 9), (50, 21)]
KINDS = ("ramp", "uniform", "checker")


@pytest.fixture(scope="module")
def qctx(pkg):
    """contexts of this module's own (the session's shared ones keep the reference table whatever happens here)"""
    made = {}

    def get(depth):
        if depth not in made:
            try:
                made[depth] = pkg.Context(0, 8, 8, depth)
            except Exception as e:
                pytest.fail(f"HIP context for 8x8x{depth} could not be created: {e}")
        ctx = made[depth]
        ctx.set_quant(None)
        for opt in (pkg.DCT3D_OPT_QUANT_FORCE_TABLE, pkg.DCT3D_OPT_EG_TWO_STEP, pkg.DCT3D_OPT_ENC_NO_RECHECK,
                    pkg.DCT3D_OPT_DEC_MARGIN):
            ctx.set_option(opt, 0)
        return ctx

    yield get
    for c in made.values():
        c.close()


def _stack(kind, w, h, depth, channels, salt):
    p = qc.pkg()

    def plane(i):
        if kind == "checker":
            z, y, x = np.meshgrid(np.arange(depth), np.arange(h), np.arange(w), indexing="ij")
            return (((x + y + z + i) % 2) * 255).astype(np.uint8)
        return p.synthetic.frames(w, h, depth, seed=0x77A1 + 97 * i + salt, frame0=3 * i + salt, kind=kind)

    return plane(0) if channels == 1 else np.stack([plane(0), plane(1), plane(2)], axis=-1)


@functools.lru_cache(maxsize=None)
def _frames(depth, channels, w, h, stacks, first):
    """stacks of content KINDS[first], KINDS[first + 1], ...: never modified"""
    fr = np.concatenate([_stack(KINDS[(first + s) % 3], w, h, depth, channels, s) for s in range(stacks)])
    fr.setflags(write=False)
    return fr


def tie_cube(depth, T):
    """A cube [depth, 8, 8] with one AC coefficient of sum s = 4 on a rounding tie of table T, so that the fp32
    certificate must leave it open whatever the content around it (random content leaves ~1e-4 to 1e-5 of the
    coefficients open: none at all in a small clip).  The coefficient's basis products are one rational number
    at the pixels used: 8x8x8, k = (0, 2, 2): with a = cos(pi/8) / 2, b = cos(3 pi/8) / 2 the 8-point row k = 2
    is (a, b, -b, -a, -a, -b, b, a), a b = sqrt(2) / 16 and the z factor 1 / (2 sqrt 2), so the 16 (y, x) with
    one index of +-a and the other of +-b of the same sign weigh +1/32 in every plane; 8x8x4, k = (0, 0, 4):
    (1/2) (1 / (2 sqrt 2)) (+-1 / (2 sqrt 2)), +1/16 at x in {0, 3, 4, 7}.  128 pixels either way; their sum
    S gives c = S / 32 (S / 16), and c / step[4] = 1/2 at S = 16 step[4] (8 step[4]) <= 128 * 255."""
    cube = np.zeros((depth, 8, 8), np.uint8)
    if depth == 8:
        A, B = (0, 7), (1, 6)      # +a, +b
        nA, nB = (3, 4), (2, 5)    # -a, -b
        pos = [(y, x) for y in A for x in B] + [(y, x) for y in B for x in A] + \
              [(y, x) for y in nA for x in nB] + [(y, x) for y in nB for x in nA]
        total = 16 * int(T[4])
    else:
        pos = [(y, x) for y in range(8) for x in (0, 3, 4, 7)]
        total = 8 * int(T[4])
    cells = [(z, y, x) for z in range(depth) for (y, x) in pos]
    assert len(cells) == 128
    base, extra = divmod(total, 128)
    for i, c in enumerate(cells):
        cube[c] = base + (1 if i < extra else 0)
    return cube


@functools.lru_cache(maxsize=None)
def _frames_with_tie(depth, channels, w, h, stacks, name):
    """_frames(.., first = 0) with tie_cube at the first cube of stack 0 (every channel)"""
    fr = _frames(depth, channels, w, h, stacks, 0).copy()
    cube = tie_cube(depth, qc.tables(depth)[name])
    if channels == 1:
        fr[:depth, :8, :8] = cube
    else:
        fr[:depth, :8, :8, :] = cube[..., None]
    fr.setflags(write=False)
    return fr


@functools.lru_cache(maxsize=8)
def _dct(depth, channels, w, h, stacks, first):
    """the oracle's fp64 DCT of the padded (planar) raster as cubes: shared by the cases' tables"""
    import oracle
    p = qc.pkg()
    pad = p.pad_frames(_frames(depth, channels, w, h, stacks, first))
    pl = pad if channels == 1 else qc.planar(pad, depth)
    d = oracle.to_cubes(qc.plan(depth).dct(pl), 8, 8, depth)
    d.setflags(write=False)
    return d


def _ref(depth, channels, w, h, stacks, first, T):
    """(frames, reference q [stack][channel][cube], reference decode of it cropped to the frames)"""
    p = qc.pkg()
    fr = _frames(depth, channels, w, h, stacks, first)
    q = p.quantize_ref(_dct(depth, channels, w, h, stacks, first), T)
    wp, hp = p.padded_size(w, h)
    F = stacks * depth
    if channels == 1:
        out = qc.ref_decode(q, wp, hp, F, T, depth)[:, :h, :w]
    else:
        out = qc.packed(qc.ref_decode(q, wp, hp, 3 * F, T, depth), depth)[:, :h, :w]
    return fr, q, np.ascontiguousarray(out)


def _ref_streams(q, depth, channels, stacks):
    import oracle
    blocks = q.reshape(stacks, channels, -1, 64 * depth)
    return [_expected(oracle, qc.pkg(), np.ascontiguousarray(blocks[:, ch]), depth) for ch in range(channels)]


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the cached arrays are read-only)


def _all_calls(ctx, fr, w, h, stacks, channels, q_for_decode, streams_for_decode):
    """every raster call family on one clip: (q host, q dev, frames host, frames dev, streams host, streams
    two-step, (frames, end bits) from streams, the same two-step)"""
    import torch
    p = qc.pkg()
    q_h = ctx.encode_frames(fr)
    d_q = torch.full((q_h.size,), -7, dtype=torch.int32, device="cuda")
    ctx.encode_frames_dev(_dev(fr), w, h, channels, stacks, d_q)
    ctx.synchronize()
    q_d = d_q.cpu().numpy().reshape(q_h.shape)
    o_h = ctx.decode_frames(q_for_decode, w, h, stacks, channels)
    d_o = torch.full(fr.shape, 0x5A, dtype=torch.uint8, device="cuda")
    ctx.decode_frames_dev(_dev(q_for_decode), w, h, channels, stacks, d_o)
    ctx.synchronize()
    o_d = d_o.cpu().numpy()
    s_h = ctx.encode_eg_frames(fr)
    e_h = ctx.decode_eg_frames([b for b, _ in streams_for_decode], w, h, stacks)
    with ctx_option(ctx, p.DCT3D_OPT_EG_TWO_STEP, 1):
        s_2 = ctx.encode_eg_frames(fr)
        e_2 = ctx.decode_eg_frames([b for b, _ in streams_for_decode], w, h, stacks)
    return q_h, q_d, o_h, o_d, s_h, s_2, e_h, e_2


CASES = [(d, ch, w, h, st) for d in (8, 4) for ch in (1, 3) for (w, h) in SHAPES for st in (1, 3)]


@pytest.mark.parametrize("name", qc.TABLE_NAMES)
@pytest.mark.parametrize("depth,channels,w,h,stacks", CASES)
def test_parity_every_call_family(pkg, qctx, depth, channels, w, h, stacks, name):
    """1 + 2: the int32 calls and the stream calls, host and device forms, fused and two-step"""
    T = qc.tables(depth)[name]
    first = (CASES.index((depth, channels, w, h, stacks)) + qc.TABLE_NAMES.index(name)) % 3
    fr, q_ref, out_ref = _ref(depth, channels, w, h, stacks, first, T)
    s_ref = _ref_streams(q_ref, depth, channels, stacks)
    ctx = qctx(depth)
    ctx.set_quant(T)
    assert np.array_equal(ctx.quant(), T)
    q_h, q_d, o_h, o_d, s_h, s_2, e_h, e_2 = _all_calls(ctx, fr, w, h, stacks, channels, q_ref, s_ref)
    assert np.array_equal(q_h, q_ref), f"{(q_h != q_ref).sum()} coefficients differ"
    assert np.array_equal(q_d, q_ref)
    assert np.array_equal(o_h, out_ref), f"{(o_h != out_ref).sum()} bytes differ"
    assert np.array_equal(o_d, out_ref)
    assert s_h == s_ref, "fused stream encode"
    assert s_2 == s_ref, "two-step stream encode"
    for (o, eb), what in ((e_h, "fused"), (e_2, "two-step")):
        assert eb == [bits for _, bits in s_ref], what
        assert np.array_equal(o, out_ref), what


@pytest.mark.parametrize("name", ["q2", "seeded"])
@pytest.mark.parametrize("w,h", [(136, 72), (50, 21)])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("depth", [8, 4])
def test_rare_paths_run_with_the_table(pkg, qctx, depth, channels, w, h, name):
    """3: the exact paths are where the product kernels have the literal 5.  With the second certificate off
    (8x8x8) every open coefficient takes the Java fold; with the decode margin widened as test_gpu_edge.py
    (0.25, int32 calls) and test_gpu_eg_frames.py (0.45, stream calls) widen it, lanes take the exact replay.
    The outputs stay the reference's and stats() reports the replays of that very call.  (The aligned grey
    stream encode's kernel reports no count, as with the reference table: dct3d.h.)"""
    T = qc.tables(depth)[name]
    stacks = 3
    fr = _frames_with_tie(depth, channels, w, h, stacks, name)  # a coefficient on a tie: open for certain
    q_ref, out_ref = qc.ref_frames(fr, T, depth)
    s_ref = _ref_streams(q_ref, depth, channels, stacks)
    ctx = qctx(depth)
    ctx.set_quant(T)
    with ctx_option(ctx, pkg.DCT3D_OPT_ENC_NO_RECHECK, 1):
        q = ctx.encode_frames(fr)
        st = ctx.stats()
        assert np.array_equal(q, q_ref), f"{(q != q_ref).sum()} coefficients differ"
        assert st["n_flagged"] > 0 and st["n_rechecked"] == 0, st
        s = ctx.encode_eg_frames(fr)
        st = ctx.stats()
        assert s == s_ref
        if channels == 3 or (w, h) == (50, 21):
            assert st["n_flagged"] > 0, st
    with ctx_option(ctx, pkg.DCT3D_OPT_DEC_MARGIN, 0.25):
        out = ctx.decode_frames(q_ref, w, h, stacks, channels)
        st = ctx.stats()
        assert st["n_flagged"] > 0, st
        assert np.array_equal(out, out_ref)
    with ctx_option(ctx, pkg.DCT3D_OPT_DEC_MARGIN, 0.45):
        out, eb = ctx.decode_eg_frames([b for b, _ in s_ref], w, h, stacks)
        st = ctx.stats()
        assert st["n_flagged"] > 0, st
        assert eb == [bits for _, bits in s_ref] and np.array_equal(out, out_ref)


@pytest.mark.parametrize("w,h", [(136, 72), (50, 21)])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("depth", [8, 4])
def test_forced_table_equals_product_kernels(pkg, qctx, depth, channels, w, h):
    """4: DCT3D_OPT_QUANT_FORCE_TABLE with no table set: the table kernels reading max(1, 5 s) from the table give
    bit for bit what the product kernels give, every call family"""
    stacks = 3
    fr = _frames(depth, channels, w, h, stacks, 0)
    ctx = qctx(depth)
    q0 = ctx.encode_frames(fr)
    s0 = ctx.encode_eg_frames(fr)
    a = _all_calls(ctx, fr, w, h, stacks, channels, q0, s0)
    with ctx_option(ctx, pkg.DCT3D_OPT_QUANT_FORCE_TABLE, 1):
        b = _all_calls(ctx, fr, w, h, stacks, channels, q0, s0)
        # and the rare paths: the fold's and the replay's divisor from the table
        with ctx_option(ctx, pkg.DCT3D_OPT_ENC_NO_RECHECK, 1):
            assert np.array_equal(ctx.encode_frames(fr), q0)
        with ctx_option(ctx, pkg.DCT3D_OPT_DEC_MARGIN, 0.25):
            assert np.array_equal(ctx.decode_frames(q0, w, h, stacks, channels), a[2])
    for x, y in zip(a[:4], b[:4]):
        assert np.array_equal(x, y)
    assert a[4] == b[4] == a[5] == b[5] == s0
    for (o, eb), (o2, eb2) in zip(a[6:], b[6:]):
        assert eb == eb2 and np.array_equal(o, o2)
    assert np.array_equal(a[0], q0)


@pytest.mark.parametrize("depth", [8, 4])
def test_state(pkg, qctx, depth):
    """5: the table is the context's state: set, encode, reset, encode -- the second result is the parent
    behaviour (the oracle's encode_q); quant() round-trips; two contexts do not disturb each other; a refused
    table changes nothing"""
    T12, T2 = qc.tables(depth)["q12"], qc.tables(depth)["q2"]
    fr = pkg.synthetic.frames(40, 24, 2 * depth, kind="uniform")
    ref0 = qc.plan(depth).encode_q(fr)
    ctx = qctx(depth)
    assert np.array_equal(ctx.quant(), pkg.quant_table(5, depth))
    ctx.set_quant(T12)
    assert np.array_equal(ctx.quant(), T12)
    assert np.array_equal(ctx.encode_stacks(fr), qc.ref_encode(fr, T12, depth))
    with pytest.raises(pkg.Dct3dError):
        ctx.set_quant(np.zeros(qc.n_steps(depth), np.int32))
    with pytest.raises(pkg.Dct3dError):
        ctx.set_quant(T12[:-1])
    assert np.array_equal(ctx.quant(), T12)
    other = pkg.Context(0, 8, 8, depth)
    try:
        other.set_quant(T2)
        assert np.array_equal(other.encode_stacks(fr), qc.ref_encode(fr, T2, depth))
        assert np.array_equal(ctx.encode_stacks(fr), qc.ref_encode(fr, T12, depth))
        assert np.array_equal(other.quant(), T2) and np.array_equal(ctx.quant(), T12)
    finally:
        other.close()
    ctx.set_quant(None)
    assert np.array_equal(ctx.quant(), pkg.quant_table(5, depth))
    assert np.array_equal(ctx.encode_stacks(fr), ref0)
    ctx.set_quant(pkg.quant_table(5, depth))  # the reference table set explicitly: the same
    assert np.array_equal(ctx.encode_stacks(fr), ref0)
    assert np.array_equal(ctx.decode_stacks(ref0, 40, 24, 2), qc.plan(depth).decode_q(ref0, 40, 24, 2 * depth))


# ---- 6: the codec CLI ------------------------------------------------------------------------------------------

def _run_cli(pkg, args, env=None):
    r = subprocess.run([pkg.CLI_PATH] + [str(a) for a in args], capture_output=True, text=True,
                       env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def _payload(q, depth, channels, stacks, ch):
    """the oracle's Exp-Golomb payload of channel ch's cubes in diagonal order (the inflated .bin)"""
    import oracle
    vals = q.reshape(stacks, channels, -1, 64 * depth)[:, ch].reshape(-1, 64 * depth)[:, qc.pkg().diagonal_order(8, 8, depth)]
    return oracle.eg_write(np.ascontiguousarray(vals).reshape(-1))


@pytest.mark.parametrize("how", ["argument", "environment", "argument_host_eg"])
@pytest.mark.parametrize("channels", [1, 3])
def test_codec_cli_with_a_quantiser(pkg, tmp_path, channels, how):
    """dct3d_codec encode / decode (encode_rgb / decode_rgb) on 16 frames of 50 x 21 with q=12, given as the 9th
    argument or in DCT3D_CODEC_QUANT, device or host Exp-Golomb: the .bin inflates to eg_write of the reference
    q, the decoded file is the reference bytes, and decoding without the quantiser gives other frames"""
    w, h, frames, depth = 50, 21, 16, 8
    T = pkg.quant_table(12, depth)
    fr = _frames(depth, channels, w, h, frames // depth, 0)
    q_ref, out_ref = qc.ref_frames(fr, T, depth)
    raw, binf, outf, plain = tmp_path / "in.raw", tmp_path / "o.bin", tmp_path / "o.raw", tmp_path / "plain.raw"
    raw.write_bytes(fr.tobytes())
    enc, dec = ("encode", "decode") if channels == 1 else ("encode_rgb", "decode_rgb")
    quant = ["q=12"] if how != "environment" else []
    env = {"DCT3D_CODEC_BATCH": "1", "DCT3D_CODEC_HOST_EG": "1" if how == "argument_host_eg" else "0"}
    if how == "environment":
        env["DCT3D_CODEC_QUANT"] = "q=12"
    _run_cli(pkg, [enc, raw, binf, w, h, frames, 1, depth] + quant, env)
    names = [str(binf)] if channels == 1 else [str(binf) + s for s in (".red", ".green", ".blue")]
    for ch, name in enumerate(names):
        assert zlib.decompress(open(name, "rb").read()) == _payload(q_ref, depth, channels, frames // depth, ch), name
    _run_cli(pkg, [dec, binf, outf, w, h, frames, 1, depth] + quant, env)
    assert np.array_equal(np.frombuffer(outf.read_bytes(), np.uint8).reshape(fr.shape), out_ref)
    # the knob is live: the same file decoded with the reference quantiser is another video
    env.pop("DCT3D_CODEC_QUANT", None)
    _run_cli(pkg, [dec, binf, plain, w, h, frames, 1, depth], env)
    assert plain.read_bytes() != outf.read_bytes()
    # the comma list of the same table: the same file
    _run_cli(pkg, [enc, raw, tmp_path / "l.bin", w, h, frames, 1, depth, ",".join(map(str, T))], env)
    for name in names:
        assert open(name, "rb").read() == open(name.replace("o.bin", "l.bin"), "rb").read()


def test_codec_cli_timing_line_prints_the_table(pkg, tmp_path):
    import json
    raw = tmp_path / "in.raw"
    raw.write_bytes(_frames(8, 1, 24, 16, 1, 0).tobytes())
    r = _run_cli(pkg, ["encode", raw, tmp_path / "o.bin", 24, 16, 8, 1, 8, "q=2"], {"DCT3D_CODEC_TIMING": "1"})
    assert json.loads(r.stderr.strip().splitlines()[-1])["quant"] == pkg.quant_table(2).tolist()
    r = _run_cli(pkg, ["decode", tmp_path / "o.bin", tmp_path / "o.raw", 24, 16, 8, 1, 8], {"DCT3D_CODEC_TIMING": "1"})
    assert json.loads(r.stderr.strip().splitlines()[-1])["quant"] == pkg.quant_table(5).tolist()


def test_codec_cli_without_a_quantiser_is_unchanged(pkg, plan8, tmp_path):
    """nothing set: the file test_gpu_codec.py expects -- the reference C encoder's entropy stage over the
    oracle's encode_q -- and q=5, the reference table given explicitly, writes the same"""
    from test_host_codec import reference_entropy_encode
    w, h, frames = 64, 64, 16
    fr = pkg.synthetic.frames(w, h, frames, kind="ramp")
    raw = tmp_path / "in.raw"
    raw.write_bytes(fr.tobytes())
    _run_cli(pkg, ["encode", raw, tmp_path / "a.bin", w, h, frames, 1], {"DCT3D_CODEC_BATCH": "2"})
    _run_cli(pkg, ["encode", raw, tmp_path / "b.bin", w, h, frames, 1, 8, "q=5"], {"DCT3D_CODEC_BATCH": "2"})
    want = reference_entropy_encode(plan8.encode_q(fr).reshape(-1), w, h, frames // 8, 8)
    assert (tmp_path / "a.bin").read_bytes() == want
    assert (tmp_path / "b.bin").read_bytes() == want


def test_codec_multi_device_with_a_quantiser(pkg, tmp_path):
    """encode_multi over the device list 1,1 at 136 x 72 with q=12 writes encode_ex's .bin, and decode_multi
    decodes it to the reference bytes"""
    w, h, frames, depth = 136, 72, 24, 8
    T = pkg.quant_table(12, depth)
    fr = _frames(depth, 1, w, h, frames // depth, 0)
    q_ref, out_ref = qc.ref_frames(fr, T, depth)
    raw, one, multi, outf = tmp_path / "in.raw", tmp_path / "one.bin", tmp_path / "multi.bin", tmp_path / "o.raw"
    raw.write_bytes(fr.tobytes())
    env = {"DCT3D_CODEC_BATCH": "1"}
    _run_cli(pkg, ["encode", raw, one, w, h, frames, "1", depth, "q=12"], env)
    _run_cli(pkg, ["encode", raw, multi, w, h, frames, "1,1", depth, "q=12"], env)
    assert multi.read_bytes() == one.read_bytes()
    assert zlib.decompress(one.read_bytes()) == _payload(q_ref, depth, 1, frames // depth, 0)
    _run_cli(pkg, ["decode", multi, outf, w, h, frames, "1,1", depth, "q=12"], env)
    assert np.array_equal(np.frombuffer(outf.read_bytes(), np.uint8).reshape(fr.shape), out_ref)
