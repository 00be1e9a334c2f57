"""CPU: the distortion probe's entry points (dct3d_distortion_frames*) are exported, declared and listed and
validate their arguments; psnr_db and pick_quality_psnr; the codec's psnr= parser and the CLI's rejections.  Nothing
here needs a device."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

DIST_SYMBOLS = ("dct3d_distortion_frames_dev", "dct3d_distortion_frames")


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_distortion_symbols_exported_declared_and_listed(pkg):
    assert set(DIST_SYMBOLS) <= _exported(pkg.LIB_PATH)
    assert set(DIST_SYMBOLS) <= set(pkg.ABI_SYMBOLS)
    header = open(os.path.join(pkg.INCLUDE_DIR, "dct3d.h")).read()
    for name in DIST_SYMBOLS:
        assert re.search(r"^int %s\(dct3d_ctx \*ctx," % name, header, re.M), name
    assert {"codec_parse_psnr", "codec_set_psnr"} <= _exported(pkg.CODEC_LIB_PATH)
    codec_h = open(os.path.join(pkg.INCLUDE_DIR, "codec.h")).read()
    for name in ("codec_parse_psnr", "codec_set_psnr"):
        assert re.search(r"^int %s\(const char \*text" % name, codec_h, re.M), name


def _args(h, n_tables=2):
    buf = (C.c_uint8 * (16 * 16 * 8 * 3))()
    tabs = (C.c_int32 * (32 * 22))(*([7] * (32 * 22)))
    sse = (C.c_uint64 * (32 * 3))()
    bits = (C.c_uint64 * (32 * 3))()
    return [h, C.cast(buf, C.c_void_p), 13, 11, 3, 1, C.cast(tabs, C.c_void_p), n_tables, C.cast(sse, C.c_void_p),
            C.cast(bits, C.c_void_p)], (buf, tabs, sse, bits)


def _with(args, i, v):
    b = list(args)
    b[i] = v
    return b


def test_null_context_is_einval(pkg):
    L = pkg.lib()
    args, keep = _args(None)
    assert L.dct3d_distortion_frames(*args) == pkg.DCT3D_EINVAL
    assert L.dct3d_distortion_frames_dev(*(args + [None])) == pkg.DCT3D_EINVAL
    assert L.dct3d_distortion_frames(None, None, 0, 0, 0, 0, None, 0, None, None) == pkg.DCT3D_EINVAL


def test_bad_arguments_with_a_device(pkg):
    """Every argument error is DCT3D_EINVAL (checked where a context can be made; here the NULL-context test
    stands); bits == NULL is no error."""
    L = pkg.lib()
    h = C.c_void_p()
    if L.dct3d_ctx_create(0, 8, 8, 8, C.byref(h)) != pkg.DCT3D_OK:
        return
    try:
        E = pkg.DCT3D_EINVAL
        for f, tail in ((L.dct3d_distortion_frames, []), (L.dct3d_distortion_frames_dev, [None])):
            args, keep = _args(h)
            for i, v in ((2, 0), (3, -1), (4, 2), (4, 0), (5, -1), (1, None), (8, None), (7, 0), (7, 33), (7, -1)):
                assert f(*(_with(args, i, v) + tail)) == E, (f.__name__, i, v)
            assert f(*(_with(_with(args, 6, None), 7, 2) + tail)) == E  # tables == NULL needs n_tables == 1
            for bad in (0, 256, -3):
                args, keep = _args(h)
                keep[1][22 + 5] = bad  # a step of the second table
                assert f(*(args + tail)) == E, bad
    finally:
        L.dct3d_ctx_destroy(h)


def test_psnr_db(pkg):
    assert pkg.psnr_db(0, 1000) == math.inf
    assert pkg.psnr_db(255 * 255 * 10, 10) == 0.0
    assert pkg.psnr_db(10, 10) == pytest.approx(20 * math.log10(255.0), rel=1e-15)
    assert pkg.psnr_db(np.uint64(650250), np.int64(100)) == pytest.approx(10.0, rel=1e-15)
    assert pkg.psnr_db(1, 2**40) > pkg.psnr_db(2, 2**40) > 0


def test_pick_quality_psnr(pkg):
    pick = pkg.pick_quality_psnr
    n = 1000
    sse = lambda db: int(round(255 * 255 * n / 10 ** (db / 10)))  # noqa: E731
    mono = {1: sse(45), 2: sse(40), 4: sse(35), 8: sse(30)}
    assert pick(mono, n, 29) == 8 and pick(mono, n, 32) == 4 and pick(mono, n, 37) == 2 and pick(mono, n, 42) == 1
    assert pick(mono, n, 50) == 1  # none reaches the target: the smallest quality
    assert pick(mono, n, pkg.psnr_db(mono[4], n)) == 4  # >=: a quality exactly at the target counts
    # no monotonicity assumed: the largest quality that reaches the target, even when a smaller one does not
    bumpy = {1: sse(40), 2: sse(31), 3: sse(36), 5: sse(29), 8: sse(33)}
    assert pick(bumpy, n, 32) == 8 and pick(bumpy, n, 35) == 3 and pick(bumpy, n, 38) == 1 and pick(bumpy, n, 30) == 8
    assert pick(bumpy, n, 60) == 1
    assert pick({64: sse(20), 3: sse(30), 16: sse(25)}, n, 22) == 16  # the dict's order does not matter
    assert pick({7: sse(30)}, n, 50) == 7
    # sse == 0: infinite PSNR reaches every target
    assert pick({1: 0, 2: sse(30), 4: 0, 8: sse(20)}, n, 1e9) == 4
    with pytest.raises(ValueError):
        pick({}, n, 5)


def _codec(pkg):
    pkg.lib()
    L = C.CDLL(pkg.CODEC_LIB_PATH)
    L.codec_parse_psnr.argtypes = [C.c_char_p, C.POINTER(C.c_double)]
    L.codec_parse_rate.argtypes = [C.c_char_p, C.POINTER(C.c_double)]
    for f in (L.codec_set_psnr, L.codec_set_rate, L.codec_set_quant):
        f.argtypes = [C.c_char_p]
    return L


def test_codec_parse_psnr(pkg):
    """the same shapes of text as codec_parse_rate, accepted and rejected"""
    L = _codec(pkg)
    v = C.c_double(-7.0)
    assert L.codec_parse_psnr(b"psnr=38.5", C.byref(v)) == 0 and v.value == 38.5
    assert L.codec_parse_psnr(b"psnr=40", C.byref(v)) == 0 and v.value == 40.0
    assert L.codec_parse_psnr(b"psnr=.25", C.byref(v)) == 0 and v.value == 0.25
    shapes = ("", "-1", "abc", "1.5x", " 1", "+1", "0", "nan", "inf", "1e2", "0x10")
    for tail in shapes:
        for parse, key in ((L.codec_parse_psnr, "psnr="), (L.codec_parse_rate, "rate=")):
            v.value = -7.0
            assert parse((key + tail).encode(), C.byref(v)) == 1, key + tail
            assert v.value == -7.0, key + tail
    for bad in (b"q=5", b"rate=1.5", b"38.5", b"", None):
        v.value = -7.0
        assert L.codec_parse_psnr(bad, C.byref(v)) == 1, bad
        assert v.value == -7.0, bad
    assert L.codec_parse_psnr(b"psnr=38.5", None) == 1


def test_codec_set_psnr_is_exclusive_with_quant_and_rate(pkg, tmp_path):
    L = _codec(pkg)
    try:
        assert L.codec_set_quant(b"q=3") == 0
        assert L.codec_set_psnr(b"psnr=38") == 1  # a quantiser is set
        assert L.codec_set_quant(None) == 0
        assert L.codec_set_rate(b"rate=1.5") == 0
        assert L.codec_set_psnr(b"psnr=38") == 1  # a rate target is set
        assert L.codec_set_rate(None) == 0
        assert L.codec_set_psnr(b"psnr=38") == 0
        assert L.codec_set_rate(b"rate=1.5") == 1  # a PSNR target is set
        assert L.codec_set_psnr(b"psnr=" + b"1" * 100) == 1  # too long: nothing changes
        assert L.codec_set_rate(b"rate=1.5") == 1
        assert L.codec_set_psnr(b"") == 0
        assert L.codec_set_rate(b"rate=1.5") == 0
    finally:
        L.codec_set_psnr(None)
        L.codec_set_rate(None)
        L.codec_set_quant(None)
    # by the environment: the call itself refuses, before it opens a file or a device
    raw = tmp_path / "in.raw"
    np.zeros(8 * 8 * 8, np.uint8).tofile(raw)
    argv = [pkg.CLI_PATH, "encode", str(raw), str(tmp_path / "o.bin"), "8", "8", "8"]
    for extra, said in (({"DCT3D_CODEC_QUANT": "q=3"}, "exclude each other"),
                        ({"DCT3D_CODEC_RATE": "rate=1.5"}, "exclude each other"),
                        ({"DCT3D_CODEC_PSNR": "psnr=abc"}, "Invalid psnr target")):
        env = dict(os.environ, DCT3D_CODEC_PSNR="psnr=38")
        env.update(extra)
        r = subprocess.run(argv, env=env, capture_output=True, text=True)
        assert r.returncode == 1 and said in r.stdout and not (tmp_path / "o.bin").exists(), r.stdout


@pytest.mark.parametrize("args,said", [
    (["decode", "IN", "OUT", "8", "8", "8", "1", "8", "psnr=38"], "psnr= applies to encode"),
    (["decode_rgb", "IN", "OUT", "8", "8", "8", "1", "8", "psnr=38"], "psnr= applies to encode"),
    (["encode", "IN", "OUT", "8", "8", "8", "1,1", "8", "psnr=38"], "psnr= applies to encode"),
    (["decode", "IN", "OUT", "8", "8", "8", "1,1", "8", "psnr=38"], "psnr= applies to encode"),
    (["encode", "IN", "OUT", "8", "8", "8", "1", "8", "q=3", "psnr=38"], "exclude each other"),
    (["encode", "IN", "OUT", "8", "8", "8", "1", "8", "psnr=38", "q=3"], "exclude each other"),
    (["encode", "IN", "OUT", "8", "8", "8", "1", "8", "rate=1.5", "psnr=38"], "exclude each other"),
    (["encode_rgb", "IN", "OUT", "8", "8", "8", "1", "4", "psnr=38", "rate=1.5"], "exclude each other"),
    (["encode_rgb", "IN", "OUT", "8", "8", "8", "1", "4", "psnr="], "Invalid psnr target"),
    (["encode", "IN", "OUT", "8", "8", "8", "1", "8", "psnr=-1"], "Invalid psnr target"),
    (["encode", "IN", "OUT", "8", "8", "8", "1", "8", "psnr=abc"], "Invalid psnr target"),
    (["encode", "IN", "OUT", "8", "8", "8", "1", "8", "psnr=inf"], "Invalid psnr target"),
])
def test_cli_rejects(pkg, tmp_path, args, said):
    """psnr= on a decode, with several devices, together with q= or rate=, or malformed: refused before any file is
    made"""
    raw = tmp_path / "in.raw"
    np.zeros(8 * 8 * 8 * 3, np.uint8).tofile(raw)
    out = tmp_path / "out.bin"
    argv = [str(raw) if a == "IN" else str(out) if a == "OUT" else a for a in args]
    r = subprocess.run([pkg.CLI_PATH] + argv, capture_output=True, text=True)
    assert r.returncode == 1 and said in r.stdout, r.stdout
    assert not out.exists() and not (tmp_path / "out.bin.red").exists()


def test_decode_entry_points_reject_a_psnr_target(pkg, tmp_path):
    """the library's decode and multi-device entry points refuse a PSNR target given by the environment"""
    raw = tmp_path / "in.bin"
    np.zeros(64, np.uint8).tofile(raw)
    env = dict(os.environ, DCT3D_CODEC_PSNR="psnr=38")
    for argv in (["decode", str(raw), str(tmp_path / "o.raw"), "8", "8", "8"],
                 ["decode", str(raw), str(tmp_path / "o.raw"), "8", "8", "8", "1,1"],
                 ["encode", str(raw), str(tmp_path / "o.raw"), "8", "8", "8", "1,1"]):
        r = subprocess.run([pkg.CLI_PATH] + argv, env=env, capture_output=True, text=True)
        assert r.returncode == 1 and "psnr= applies to single-device encodes only" in r.stdout, r.stdout
        assert not (tmp_path / "o.raw").exists()
