"""CPU: the RGB and luma SSIM probe's entry points (dct3d_ssim_rgb_frames*) are exported, declared and
listed and validate their arguments; pick_stack_channel_qualities_ssim against a brute-force restatement; the codec's
ssim_rgb= parser, its exclusions and the CLI's rejections; ssim= with ycc=1 is still refused with its old words.  One
test, marked gpu, needs a device: the argument errors behind the context check."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

RGB_SYMBOLS = ("dct3d_ssim_rgb_frames_dev", "dct3d_ssim_rgb_frames")
CODEC_SYMBOLS = ("codec_parse_ssim_rgb", "codec_set_ssim_rgb")


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_symbols_exported_declared_and_listed(pkg):
    assert set(RGB_SYMBOLS) <= _exported(pkg.LIB_PATH)
    assert set(RGB_SYMBOLS) <= set(pkg.ABI_SYMBOLS)
    header = open(os.path.join(pkg.INCLUDE_DIR, "dct3d.h")).read()
    for name in RGB_SYMBOLS:
        assert re.search(r"^int %s\(dct3d_ctx \*ctx," % name, header, re.M), name
    assert set(CODEC_SYMBOLS) <= _exported(pkg.CODEC_LIB_PATH)
    codec_h = open(os.path.join(pkg.INCLUDE_DIR, "codec.h")).read()
    for name in CODEC_SYMBOLS:
        assert re.search(r"^int %s\(const char \*text" % name, codec_h, re.M), name
    assert hasattr(pkg.Context, "ssim_rgb_frames") and hasattr(pkg.Context, "ssim_rgb_frames_dev")
    assert callable(pkg.pick_stack_channel_qualities_ssim)


def _args(h, n_tables=2, n_cand=2):
    """[ctx, frames, w, h, n_stacks, tables, n_tables, cand, n_cand, ssim, ssim_y, sse, bits]"""
    buf = (C.c_uint8 * (16 * 16 * 8 * 3))()
    tabs = (C.c_int32 * (32 * 22))(*([7] * (32 * 22)))
    cand = (C.c_uint8 * (3 * 33))(*([0, 1, 0] * 33))
    ssim = (C.c_int64 * (64 * 3))()
    ssim_y = (C.c_int64 * 64)()
    sse = (C.c_uint64 * 64)()
    bits = (C.c_uint64 * (32 * 3))()
    vp = C.c_void_p
    return [h, C.cast(buf, vp), 13, 11, 1, C.cast(tabs, vp), n_tables, C.cast(cand, vp), n_cand, C.cast(ssim, vp),
            C.cast(ssim_y, vp), C.cast(sse, vp), C.cast(bits, vp)], (buf, tabs, cand, ssim, ssim_y, sse, bits)


def _with(args, i, v):
    b = list(args)
    b[i] = v
    return b


def test_null_context_is_einval(pkg):
    L = pkg.lib()
    args, keep = _args(None)
    assert L.dct3d_ssim_rgb_frames(*args) == pkg.DCT3D_EINVAL
    assert L.dct3d_ssim_rgb_frames_dev(*(args + [None])) == pkg.DCT3D_EINVAL
    assert L.dct3d_ssim_rgb_frames(None, None, 0, 0, 0, None, 0, None, 0, None, None, None, None) == pkg.DCT3D_EINVAL
    # every bad argument of the list below, on a NULL context: still DCT3D_EINVAL, nothing is dereferenced
    for i, v in ((2, 0), (4, -1), (1, None), (9, None), (6, 0), (6, 33), (8, 0), (8, 33)):
        assert L.dct3d_ssim_rgb_frames(*_with(args, i, v)) == pkg.DCT3D_EINVAL
        assert L.dct3d_ssim_rgb_frames_dev(*(_with(args, i, v) + [None])) == pkg.DCT3D_EINVAL


@pytest.mark.gpu
def test_bad_arguments_with_a_device(pkg):
    """Every argument error that needs a context is DCT3D_EINVAL, through the C-ABI itself (the one test of this module
    that needs a device), after the same arguments without the error are accepted, with every optional pointer NULL
    too.  ssim_y in planes mode is among the errors; under the colour transform it is accepted."""
    L = pkg.lib()
    h = C.c_void_p()
    assert L.dct3d_ctx_create(0, 8, 8, 8, C.byref(h)) == pkg.DCT3D_OK
    try:
        E = pkg.DCT3D_EINVAL
        # (the host-pointer call alone: the frames of _args are host memory)
        args, keep = _args(h)
        ok = _with(args, 10, None)  # planes mode: no ssim_y
        assert L.dct3d_ssim_rgb_frames(*ok) == pkg.DCT3D_OK  # the arguments every case below spoils
        assert L.dct3d_ssim_rgb_frames(*_with(_with(ok, 11, None), 12, None)) == pkg.DCT3D_OK
        for f, tail in ((L.dct3d_ssim_rgb_frames, []), (L.dct3d_ssim_rgb_frames_dev, [None])):
            args, keep = _args(h)
            ok = _with(args, 10, None)
            assert f(*(args + tail)) == E, "ssim_y in planes mode"
            # what the rate probe's check refuses; ssim == NULL; n_cand outside 1..32
            for i, v in ((2, 0), (3, -1), (4, -1), (1, None), (9, None), (6, 0), (6, 33), (6, -1), (8, 0), (8, 33), (8, -1)):
                assert f(*(_with(ok, i, v) + tail)) == E, (f.__name__, i, v)
            assert f(*(_with(_with(ok, 5, None), 6, 2) + tail)) == E  # tables == NULL needs n_tables == 1
            assert f(*(_with(_with(ok, 7, None), 8, 3) + tail)) == E  # cand == NULL needs n_cand == n_tables
            for bad in (0, 256, -3):
                args, keep = _args(h)
                keep[1][22 + 5] = bad  # a step of the second table
                assert f(*(_with(args, 10, None) + tail)) == E, bad
            args, keep = _args(h)
            keep[2][4] = 2  # a candidate index >= n_tables
            assert f(*(_with(args, 10, None) + tail)) == E
            # 4:2:0 without the colour transform
            args, keep = _args(h)
            assert L.dct3d_ctx_set_chroma(h, pkg.DCT3D_CHROMA_420) == pkg.DCT3D_OK
            try:
                assert f(*(_with(args, 10, None) + tail)) == E
            finally:
                L.dct3d_ctx_set_chroma(h, pkg.DCT3D_CHROMA_444)
        # under the colour transform ssim_y is taken
        args, keep = _args(h)
        assert L.dct3d_ctx_set_option(h, pkg.DCT3D_OPT_COLOUR, C.c_double(pkg.DCT3D_COLOUR_YCBCR)) == pkg.DCT3D_OK
        assert L.dct3d_ssim_rgb_frames(*args) == pkg.DCT3D_OK
        assert any(keep[4])
    finally:
        L.dct3d_ctx_destroy(h)


def test_context_methods_refuse_wrong_shapes_before_the_library(pkg):
    """grey frames and a malformed candidate list never reach the library (no context needed to see it)"""
    ctx = object.__new__(pkg.Context)
    ctx._h, ctx.bw, ctx.bh, ctx.bd = None, 8, 8, 8
    try:
        with pytest.raises(pkg.Dct3dError) as e:
            ctx.ssim_rgb_frames(np.zeros((8, 8, 8), np.uint8))
        assert e.value.code == pkg.DCT3D_EINVAL
        for bad in ([(0, 0)], [[0, 0, 256]], [[0, -1, 0]], []):
            with pytest.raises(pkg.Dct3dError) as e:
                ctx.ssim_rgb_frames(np.zeros((8, 8, 8, 3), np.uint8), None, bad)
            assert e.value.code == pkg.DCT3D_EINVAL
    finally:
        ctx._h = None


def _brute(pkg, ssim, qualities, n, target, rungs):
    """the rule restated: per stack, over the candidates (q_i, q_j, q_j), the largest q_i whose mean over R, G and B
    reaches the target; else the smallest q_i"""
    T = len(qualities)
    res = []
    for s in range(ssim.shape[1]):
        ok = [qualities[i] for i in range(T) if sum(int(v) for v in ssim[i, s]) / (16777216.0 * n) >= target]
        q = max(ok) if ok else min(qualities)
        i = qualities.index(q)
        j = min(i + rungs, T - 1)
        res.append((q, qualities[j], qualities[j]))
    return res


def test_pick_stack_channel_qualities_ssim(pkg):
    pick = pkg.pick_stack_channel_qualities_ssim
    n = 3 * 15 * 11 * 8  # the windows of one stack: three planes of 61 x 45, 8 frames
    at = lambda m: [int(m * 16777216 * n) // 3 + 1] * 3  # noqa: E731  (a stack's three sums of mean m, rounded up)
    q = [1, 2, 4, 8, 16]
    mono = np.array([[at(0.99), at(0.98)], [at(0.95), at(0.96)], [at(0.90), at(0.91)], [at(0.80), at(0.79)], [at(0.5), at(0.4)]], np.int64)
    assert mono.shape == (5, 2, 3)
    assert pick(mono, q, n, 0.85) == [(4, 4, 4), (4, 4, 4)]
    assert pick(mono, q, n, 0.85, 2) == [(4, 16, 16), (4, 16, 16)]
    assert pick(mono, q, n, 0.795, 1) == [(8, 16, 16), (4, 8, 8)]
    assert pick(mono, q, n, 1.0) == [(1, 1, 1), (1, 1, 1)]  # none reaches it: the smallest
    assert pick(mono, q, n, 0.01, 3) == [(16, 16, 16), (16, 16, 16)]  # j is clipped to the last rung
    # non-monotone sums (negative ones among them), every target, every offset: the brute-force restatement
    rng = np.random.default_rng(20261021)
    for trial in range(20):
        T = int(rng.integers(1, 7))
        quals = sorted(rng.choice(np.arange(1, 65), T, replace=False).tolist())
        if trial % 3 == 0:
            quals = quals[::-1]  # the order of the list does not matter to the rule
        ssim = rng.integers(-(1 << 24) * (n // 3) // 8, (1 << 24) * (n // 3) + 1, (T, 4, 3))
        for target, rungs in itertools.product((0.05, 0.3, 0.5, 0.77, 1.0), (0, 1, 2, 7)):
            assert pick(ssim, quals, n, target, rungs) == _brute(pkg, ssim, quals, n, target, rungs)
    full = [(1 << 24) * (n // 3)] * 3
    assert pick(np.array([[full], [at(0.3)], [full]]), [1, 2, 3], n, 1.0) == [(3, 3, 3)]  # x == y reaches every target
    for bad in (lambda: pick(mono[:4], q, n, 0.9), lambda: pick(mono[..., 0], q, n, 0.9), lambda: pick(mono[..., :2], q, n, 0.9),
                lambda: pick(mono, q, n, 0.9, -1), lambda: pick(mono, q, n, 0.9, 0.5)):
        with pytest.raises(ValueError):
            bad()


def _codec(pkg):
    pkg.lib()
    L = C.CDLL(pkg.CODEC_LIB_PATH)
    for f in (L.codec_parse_ssim_rgb, L.codec_parse_ssim):
        f.argtypes = [C.c_char_p, C.POINTER(C.c_double)]
    for f in (L.codec_set_ssim_rgb, L.codec_set_ssim, L.codec_set_psnr_rgb, L.codec_set_psnr, L.codec_set_rate, L.codec_set_quant):
        f.argtypes = [C.c_char_p]
    return L


def test_codec_parse_ssim_rgb(pkg):
    L = _codec(pkg)
    v = C.c_double(-7.0)
    assert L.codec_parse_ssim_rgb(b"ssim_rgb=0.95", C.byref(v)) == 0 and v.value == 0.95
    assert L.codec_parse_ssim_rgb(b"ssim_rgb=1", C.byref(v)) == 0 and v.value == 1.0
    assert L.codec_parse_ssim_rgb(b"ssim_rgb=1.0", C.byref(v)) == 0 and v.value == 1.0
    assert L.codec_parse_ssim_rgb(b"ssim_rgb=.25", C.byref(v)) == 0 and v.value == 0.25
    for tail in ("", "-1", "abc", "0.5x", " 1", "+1", "0", "0.0", "nan", "inf", "1e-2", "0x1", "1.0000001", "2"):
        v.value = -7.0
        assert L.codec_parse_ssim_rgb(("ssim_rgb=" + tail).encode(), C.byref(v)) == 1, tail
        assert v.value == -7.0, tail
    for bad in (b"q=5", b"ssim=0.9", b"psnr_rgb=38.5", b"rate=1.5", b"0.9", b"", None):
        v.value = -7.0
        assert L.codec_parse_ssim_rgb(bad, C.byref(v)) == 1, bad
        assert v.value == -7.0, bad
    assert L.codec_parse_ssim_rgb(b"ssim_rgb=0.5", None) == 1
    # the plane probe's parser does not take the new text
    assert L.codec_parse_ssim(b"ssim_rgb=0.9", C.byref(v)) == 1


def test_codec_set_ssim_rgb_is_exclusive(pkg, tmp_path):
    L = _codec(pkg)
    setters = (L.codec_set_ssim_rgb, L.codec_set_ssim, L.codec_set_psnr_rgb, L.codec_set_psnr, L.codec_set_rate, L.codec_set_quant)
    try:
        for other, text in ((L.codec_set_quant, b"q=3"), (L.codec_set_rate, b"rate=1.5"), (L.codec_set_psnr, b"psnr=38"),
                            (L.codec_set_psnr_rgb, b"psnr_rgb=38"), (L.codec_set_ssim, b"ssim=0.9")):
            assert other(text) == 0
            assert L.codec_set_ssim_rgb(b"ssim_rgb=0.9") == 1, text  # another selector is set
            assert other(None) == 0
        assert L.codec_set_ssim_rgb(b"ssim_rgb=0.9") == 0
        assert L.codec_set_rate(b"rate=1.5") == 1 and L.codec_set_ssim(b"ssim=0.9") == 1  # the RGB SSIM target is set
        assert L.codec_set_ssim_rgb(b"ssim_rgb=" + b"1" * 100) == 1  # too long: nothing changes
        assert L.codec_set_ssim(b"ssim=0.9") == 1
        assert L.codec_set_ssim_rgb(b"") == 0
        assert L.codec_set_ssim(b"ssim=0.9") == 0
    finally:
        for f in setters:
            f(None)
    # by the environment: the call itself refuses, before it opens a file or a device
    raw = tmp_path / "in.raw"
    np.zeros(8 * 8 * 8 * 3, np.uint8).tofile(raw)
    rgb = [pkg.CLI_PATH, "encode_rgb", str(raw), str(tmp_path / "o"), "8", "8", "8"]
    grey = [pkg.CLI_PATH, "encode", str(raw), str(tmp_path / "o"), "8", "8", "8"]
    for argv, extra, said in ((rgb, {"DCT3D_CODEC_QUANT": "q=3"}, "exclude each other"),
                              (rgb, {"DCT3D_CODEC_RATE": "rate=1.5"}, "exclude each other"),
                              (rgb, {"DCT3D_CODEC_PSNR": "psnr=38"}, "exclude each other"),
                              (rgb, {"DCT3D_CODEC_PSNR_RGB": "psnr_rgb=38"}, "exclude each other"),
                              (rgb, {"DCT3D_CODEC_SSIM": "ssim=0.9"}, "exclude each other"),
                              (rgb, {"DCT3D_CODEC_SSIM_RGB": "ssim_rgb=abc"}, "Invalid ssim_rgb target"),
                              (rgb, {"DCT3D_CODEC_SSIM_RGB": "ssim_rgb=1.5"}, "Invalid ssim_rgb target"),
                              (rgb, {"DCT3D_CODEC_HOST_EG": "1"}, "ssim_rgb= needs the device stream calls"),
                              (grey, {}, "ssim_rgb= applies to encode_rgb")):
        env = dict(os.environ, DCT3D_CODEC_SSIM_RGB="ssim_rgb=0.9")
        env.update(extra)
        r = subprocess.run(argv, env=env, capture_output=True, text=True)
        assert r.returncode == 1 and said in r.stdout, r.stdout
        assert not any(p.name.startswith("o") for p in tmp_path.iterdir()), r.stdout


ONE = ["8", "8", "8", "1", "8"]


@pytest.mark.parametrize("args,said", [
    (["decode_rgb", "IN", "OUT"] + ONE + ["ssim_rgb=0.9"], "ssim_rgb= applies to encode_rgb on one device"),
    (["decode", "IN", "OUT"] + ONE + ["ssim_rgb=0.9"], "ssim_rgb= applies to encode_rgb on one device"),
    (["encode", "IN", "OUT"] + ONE + ["ssim_rgb=0.9"], "ssim_rgb= applies to encode_rgb on one device"),
    (["encode_rgb", "IN", "OUT", "8", "8", "8", "1,1", "8", "ssim_rgb=0.9"], "ssim_rgb= applies to encode_rgb on one device"),
    (["encode_rgb", "IN", "OUT"] + ONE + ["q=3", "ssim_rgb=0.9"], "q= and ssim_rgb= exclude each other"),
    (["encode_rgb", "IN", "OUT"] + ONE + ["ssim_rgb=0.9", "q=3"], "q= and ssim_rgb= exclude each other"),
    (["encode_rgb", "IN", "OUT"] + ONE + ["rate=1.5", "ssim_rgb=0.9"], "rate= and ssim_rgb= exclude each other"),
    (["encode_rgb", "IN", "OUT"] + ONE + ["ssim_rgb=0.9", "psnr=38"], "psnr= and ssim_rgb= exclude each other"),
    (["encode_rgb", "IN", "OUT"] + ONE + ["psnr_rgb=38", "ssim_rgb=0.9"], "psnr_rgb= and ssim_rgb= exclude each other"),
    (["encode_rgb", "IN", "OUT"] + ONE + ["ssim_rgb=0.9", "ssim=0.9"], "ssim= and ssim_rgb= exclude each other"),
    (["encode_rgb", "IN", "OUT"] + ONE + ["ssim_rgb="], "Invalid ssim_rgb target"),
    (["encode_rgb", "IN", "OUT"] + ONE + ["ssim_rgb=0"], "Invalid ssim_rgb target"),
    (["encode_rgb", "IN", "OUT"] + ONE + ["ssim_rgb=1.01"], "Invalid ssim_rgb target"),
    (["encode_rgb", "IN", "OUT"] + ONE + ["ssim_rgb=abc"], "Invalid ssim_rgb target"),
    (["encode_rgb", "IN", "OUT"] + ONE + ["ssim_rgb=0.9", "ycc=1", "qmap=MAP", "cq=1"], "cq= applies to an encode_rgb with"),
    (["encode_rgb", "IN", "OUT"] + ONE + ["ssim_rgb=0.9", "ycc=1", "cq=1"], "cq= applies to an encode_rgb with"),
    (["encode_rgb", "IN", "OUT"] + ONE + ["ssim_rgb=0.9", "qmap3=MAP", "cq=1"], "cq= needs ycc=1"),
    (["encode_rgb", "IN", "OUT"] + ONE + ["ssim_rgb=0.9", "chroma=420"], "chroma=420 needs ycc=1"),
    # the old refusals of the plane probe's target, word for word
    (["encode_rgb", "IN", "OUT"] + ONE + ["ssim=0.9", "ycc=1"],
     "ycc=1 and ssim= exclude each other: the SSIM probe measures the R, G, B planes (luma SSIM is not built)"),
    (["encode_rgb", "IN", "OUT"] + ONE + ["ssim=0.9", "ycc=1", "chroma=420"],
     "ycc=1 and ssim= exclude each other: the SSIM probe measures the R, G, B planes (luma SSIM is not built)"),
])
def test_cli_rejects(pkg, tmp_path, args, said):
    """ssim_rgb= on a decode, on a grey command, with several devices, together with q=, rate=, psnr=, psnr_rgb= or
    ssim=, malformed, or with a cq= that has no three-column map: refused before any file is made"""
    raw = tmp_path / "in.raw"
    np.zeros(8 * 8 * 8 * 3, np.uint8).tofile(raw)
    out = tmp_path / "out.bin"
    argv = [str(raw) if a == "IN" else str(out) if a == "OUT" else a.replace("MAP", str(tmp_path / "map.txt")) for a in args]
    r = subprocess.run([pkg.CLI_PATH] + argv, capture_output=True, text=True)
    assert r.returncode == 1 and said in r.stdout, r.stdout
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.raw"], r.stdout


def test_the_old_ssim_refusal_by_the_library(pkg, tmp_path):
    """ycc=1 by the environment beside ssim=: the library's own message is the old one"""
    raw = tmp_path / "in.raw"
    np.zeros(8 * 8 * 8 * 3, np.uint8).tofile(raw)
    env = dict(os.environ, DCT3D_CODEC_YCC="1")
    r = subprocess.run([pkg.CLI_PATH, "encode_rgb", str(raw), str(tmp_path / "o"), "8", "8", "8", "1", "8", "ssim=0.9"],
                       env=env, capture_output=True, text=True)
    assert r.returncode == 1, r.stdout
    assert "ycc=1 and ssim= exclude each other: the SSIM probe measures the R, G, B planes (luma SSIM is not built)" in r.stdout
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.raw"]


def test_decode_entry_points_reject_the_target(pkg, tmp_path):
    """the library's decode and multi-device entry points refuse the target given by the environment"""
    raw = tmp_path / "in.bin"
    np.zeros(64, np.uint8).tofile(raw)
    env = dict(os.environ, DCT3D_CODEC_SSIM_RGB="ssim_rgb=0.9")
    for argv in (["decode", str(raw), str(tmp_path / "o.raw"), "8", "8", "8"],
                 ["decode_rgb", str(raw), str(tmp_path / "o.raw"), "8", "8", "8"],
                 ["decode", str(raw), str(tmp_path / "o.raw"), "8", "8", "8", "1,1"],
                 ["encode", str(raw), str(tmp_path / "o.raw"), "8", "8", "8", "1,1"]):
        r = subprocess.run([pkg.CLI_PATH] + argv, env=env, capture_output=True, text=True)
        assert r.returncode == 1 and "ssim_rgb= applies to single-device encodes only" in r.stdout, (argv, r.stdout)
        assert not (tmp_path / "o.raw").exists()
