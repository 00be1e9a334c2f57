"""GPU: the rate probe (dct3d_rate_frames*) -- the exact Exp-Golomb size of every stack and cube under
several quantiser tables from one transform -- and the codec's rate= argument built on it.

The reference is independent of csrc/: quant_common.ref_frames (the oracle's Java-semantics DCT with the numpy
quantiser) gives the cubes [stack][channel][cube], quant_common.code_bits their code widths; summed per cube and
per (stack, channel)."""
import functools
import re
import subprocess

import numpy as np
import pytest

import quant_common as qc
from test_gpu_edge import _rare_content

pytestmark = pytest.mark.gpu

LADDER = (1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 24, 32, 40, 48, 64)

# name -> (width, height, channels, stacks)
GEOMS = {
    "g64x64": (64, 64, 1, 2),
    "g61x45": (61, 45, 1, 3),
    "rgb61x45": (61, 45, 3, 3),
    "g8x8": (8, 8, 1, 3),     # one cube per stack
    "g24x24": (24, 24, 1, 2),  # 9 cubes per stack: a wave straddles the stacks, the last wave is ragged
    "rare": (29, 7, 1, 48),
    "rare_rgb": (29, 7, 3, 48),
}


def _ctx(depth, gpu_ctx8, gpu_ctx4):
    return gpu_ctx8 if depth == 8 else gpu_ctx4


@functools.lru_cache(maxsize=None)
def _frames(depth, geom):
    p = qc.pkg()
    w, h, channels, stacks = GEOMS[geom]
    if geom.startswith("rare"):
        fr = _rare_content(p, depth, channels)
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


@functools.lru_cache(maxsize=None)
def _ref_cube_bits(depth, geom, name):
    """int64 [stacks, channels, cubes per stack and channel]: the reference's bits of every cube under the table"""
    w, h, channels, stacks = GEOMS[geom]
    q = qc.ref_frames(_frames(depth, geom), _table(depth, name), depth)[0]
    b = qc.code_bits(q).reshape(q.shape[0], -1).sum(axis=1)
    b = b.reshape(stacks, channels, -1)
    b.setflags(write=False)
    return b


def _ref(depth, geom, names):
    return np.stack([_ref_cube_bits(depth, geom, n) for n in names])


def _rate_dev(ctx, depth, geom, names):
    """rate_frames_dev with a guarded cube map -> (bits [T, stacks, channels], cube bits [T, stacks, channels, C])"""
    import torch
    w, h, channels, stacks = GEOMS[geom]
    wp, hp = qc.pkg().padded_size(w, h)
    C = (wp // 8) * (hp // 8)
    n = len(names) * stacks * channels * C * 2
    buf, mid = qc.banded(torch, n, 0xA5)
    d_fr = torch.from_numpy(np.array(_frames(depth, geom))).cuda()
    bits = ctx.rate_frames_dev(d_fr, w, h, channels, stacks, [_table(depth, x) for x in names], mid)
    got, intact = qc.bands_intact(buf, n, 0xA5)
    assert intact, "a write outside d_cube_bits"
    return bits, got.view(np.uint16).reshape(len(names), stacks, channels, C)


def _assert_equal_to_reference(bits, cubes, ref, names):
    for t, name in enumerate(names):
        assert np.array_equal(cubes[t].astype(np.int64), ref[t]), \
            f"table {name}: {(cubes[t] != ref[t]).sum()} cubes differ from the reference"
        assert np.array_equal(bits[t].astype(np.int64), ref[t].sum(axis=-1)), f"table {name}: the per-stack sums differ"


@pytest.mark.parametrize("n_tables", [1, 8, 11])
@pytest.mark.parametrize("geom", ["g64x64", "g61x45", "rgb61x45", "g8x8", "g24x24"])
@pytest.mark.parametrize("depth", [8, 4])
def test_bits_equal_the_reference(gpu_ctx8, gpu_ctx4, depth, geom, n_tables):
    """1: per stack and channel, and per cube, the probe's bits are the reference's, for 1, 8 and 11 (two launches)
    tables; nothing is written outside the cube map."""
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    names = TABLE_SETS[n_tables]
    bits, cubes = _rate_dev(ctx, depth, geom, names)
    _assert_equal_to_reference(bits, cubes, _ref(depth, geom, names), names)
    w, h, channels, stacks = GEOMS[geom]
    assert ctx.stats()["n_units"] == cubes[0].size * 64 * depth * n_tables
    # the host call: the same numbers
    host = ctx.rate_frames(_frames(depth, geom), [_table(depth, x) for x in names])
    assert np.array_equal(host, bits)


@pytest.mark.parametrize("depth", [8, 4])
def test_host_call_in_several_chunks(gpu_ctx8, gpu_ctx4, depth):
    """1b: 40 frames of 1920 x 1080 (79 MiB) go up in two chunks of whole stacks on the host-pointer path (5 stacks
    as 4 + 1, 10 as 8 + 2): every (table, stack) sum lands at its place (the device call's numbers), and the chunks'
    statistics add up."""
    import torch
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    w, h, stacks = 1920, 1080, 40 // depth
    fr = np.random.default_rng(20261020).integers(0, 256, (40, h, w), dtype=np.uint8)
    fr[8:16] //= 4  # stacks that differ in what they cost
    tabs = [_table(depth, "q2"), _table(depth, "q12")]
    bits = ctx.rate_frames_dev(torch.from_numpy(fr).cuda(), w, h, 1, stacks, tabs)
    dev = ctx.stats()
    assert dev["n_units"] == 2 * fr.size
    host = ctx.rate_frames(fr, tabs)
    st = ctx.stats()
    assert st["n_units"] == 2 * fr.size
    assert st["n_flagged"] == dev["n_flagged"]
    assert np.array_equal(host, bits)
    assert len(set(int(v) for v in bits[0, :, 0])) == stacks  # no two stacks alike: a misplaced chunk would show


@pytest.mark.parametrize("geom", ["rare", "rare_rgb"])
@pytest.mark.parametrize("depth", [8, 4])
def test_rare_path(gpu_ctx8, gpu_ctx4, depth, geom):
    """2: content whose coefficients the fp32 certificate leaves open: the exact folds settle them (n_flagged > 0),
    the bits are still the reference's, and with one table the count is the stream encode's own."""
    import torch
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    w, h, channels, stacks = GEOMS[geom]
    bits, cubes = _rate_dev(ctx, depth, geom, RARE_TABLES)
    flagged = ctx.stats()["n_flagged"]
    _assert_equal_to_reference(bits, cubes, _ref(depth, geom, RARE_TABLES), RARE_TABLES)
    assert flagged > 0, "the content must leave coefficients to the exact fold"
    fr = _frames(depth, geom)
    d_fr = torch.from_numpy(np.array(fr)).cuda()
    per_table = []
    try:
        for name in ("ref", "q1"):
            one = ctx.rate_frames_dev(d_fr, w, h, channels, stacks, [_table(depth, name)])
            n_rate = ctx.stats()["n_flagged"]
            assert np.array_equal(one[0], bits[RARE_TABLES.index(name)])
            ctx.set_quant(_table(depth, name))
            caps = [int(b) // 8 + 64 for b in one[0].sum(axis=0)]
            caps = [(c + 3) // 4 * 4 for c in caps]
            outs = [torch.zeros(c, dtype=torch.uint8, device="cuda") for c in caps]
            tb = ctx.encode_eg_frames_dev(d_fr, w, h, channels, stacks, outs, caps)
            n_enc = ctx.stats()["n_flagged"]
            assert tb == [int(b) for b in one[0].sum(axis=0)]
            assert n_rate == n_enc, f"table {name}: the probe folded {n_rate} values, the stream encode {n_enc}"
            per_table.append(n_rate)
    finally:
        ctx.set_quant(None)
    assert per_table[0] > 0, "open under the reference table (tests/test_eg_frames_rare_content.py)"


@pytest.mark.parametrize("depth", [8, 4])
def test_agrees_with_the_encoder(gpu_ctx8, gpu_ctx4, depth):
    """3: for each of the 8 tables, set_quant + encode_eg_frames with non-zero carries appends exactly the probe's
    bits to every channel's stream."""
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    fr = _frames(depth, "rgb61x45")
    bits = ctx.rate_frames(fr, [_table(depth, x) for x in TABLES8])
    carry = [(0xA0, 3), (0xFF, 7), (0x40, 1)]
    try:
        for t, name in enumerate(TABLES8):
            ctx.set_quant(_table(depth, name))
            res = ctx.encode_eg_frames(fr, carry=carry)
            for ch in range(3):
                assert res[ch][1] - carry[ch][1] == int(bits[t].sum(axis=0)[ch]), f"table {name}, channel {ch}"
    finally:
        ctx.set_quant(None)


@pytest.mark.parametrize("depth", [8, 4])
def test_context_state(gpu_ctx8, gpu_ctx4, depth):
    """4: a rate call leaves the context as it was: the quantiser, the next encode's bytes; tables=None is the
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
        none = ctx.rate_frames(fr)
        assert np.array_equal(ctx.quant(), before_q)
        assert np.array_equal(none, ctx.rate_frames(fr, [_table(depth, "q2")]))
        assert np.array_equal(none[0].astype(np.int64), _ref_cube_bits(depth, geom, "q2").sum(axis=-1))
        ctx.rate_frames(fr, others)
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
            mid = ctx.rate_frames_dev(d_fr, w, h, channels, stacks, others)
            tb1 = ctx.encode_eg_frames_dev(d_fr, w, h, channels, stacks, outs[1], caps)
            ctx.synchronize()
        for tb, o in ((tb0, outs[0]), (tb1, outs[1])):
            assert tb == [bits for _, bits in before]
            for ch, (b, _) in enumerate(before):
                assert o[ch].cpu().numpy()[:len(b)].tobytes() == b
        assert np.array_equal(mid[0].astype(np.int64), _ref_cube_bits(depth, geom, "q1").sum(axis=-1))
    finally:
        ctx.synchronize()
        ctx.set_stream(None)
        ctx.set_quant(None)


def _cli(pkg, *args):
    r = subprocess.run([pkg.CLI_PATH] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@pytest.mark.parametrize("rate", ["2.0", "0.01"])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("depth", [8, 4])
def test_codec_rate(pkg, gpu_ctx8, gpu_ctx4, tmp_path, depth, channels, rate):
    """5: dct3d_codec encode / encode_rgb with rate=: the printed q=<n> is the pick rule's over the ladder's totals
    (Context.rate_frames), the files are those of the explicit q=<n>, and decode ... q=<n> returns the reference's
    frames; at rate=0.01 nothing fits and the pick is 64."""
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    w, h, frames = 61, 45, 16
    planes = [pkg.synthetic.frames(w, h, frames, seed=0xC0DEC + ch, frame0=ch, kind="ramp" if ch else "uniform")
              for ch in range(channels)]
    fr = np.ascontiguousarray(planes[0] if channels == 1 else np.stack(planes, axis=-1), np.uint8)
    totals = ctx.rate_frames(fr, [pkg.quant_table(q, depth) for q in LADDER]).sum(axis=(1, 2))
    per_q = {q: int(totals[i]) for i, q in enumerate(LADDER)}
    target = float(rate) * float(w) * float(h) * float(frames)
    want = pkg.pick_quality(per_q, target)
    if rate == "0.01":
        assert all(b > target for b in per_q.values()) and want == 64

    raw = tmp_path / "in.raw"
    fr.tofile(raw)
    enc, dec = ("encode", "decode") if channels == 1 else ("encode_rgb", "decode_rgb")
    suffixes = [""] if channels == 1 else [".red", ".green", ".blue"]
    out = _cli(pkg, enc, raw, tmp_path / "r.bin", w, h, frames, 1, depth, f"rate={rate}")
    m = re.search(r"^rate: q=(\d+) bits=(\d+)$", out, re.M)
    assert m, out
    n = int(m.group(1))
    assert n == want and int(m.group(2)) == per_q[n]
    _cli(pkg, enc, raw, tmp_path / "q.bin", w, h, frames, 1, depth, f"q={n}")
    for sfx in suffixes:
        a, b = (tmp_path / ("r.bin" + sfx)).read_bytes(), (tmp_path / ("q.bin" + sfx)).read_bytes()
        assert a == b and len(a) > 0, f"rate={rate} and q={n} wrote different files{sfx}"
    _cli(pkg, dec, tmp_path / "r.bin", tmp_path / "out.raw", w, h, frames, 1, depth, f"q={n}")
    got = np.fromfile(tmp_path / "out.raw", np.uint8).reshape(fr.shape)
    assert np.array_equal(got, qc.ref_frames(fr, pkg.quant_table(n, depth), depth)[1])
