"""CPU: the rate probe's entry points (dct3d_rate_frames*) are exported, declared and listed and validate their
arguments; pick_quality; the codec's rate= parser and the CLI's rejections.  Nothing here needs a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

RATE_SYMBOLS = ("dct3d_rate_frames_dev", "dct3d_rate_frames")


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_rate_symbols_exported_declared_and_listed(pkg):
    assert set(RATE_SYMBOLS) <= _exported(pkg.LIB_PATH)
    assert set(RATE_SYMBOLS) <= set(pkg.ABI_SYMBOLS)
    header = open(os.path.join(pkg.INCLUDE_DIR, "dct3d.h")).read()
    for name in RATE_SYMBOLS:
        assert re.search(r"^int %s\(dct3d_ctx \*ctx," % name, header, re.M), name
    assert re.search(r"^#define DCT3D_RATE_MAX_TABLES 32$", header, re.M)
    assert pkg.RATE_MAX_TABLES == 32
    assert {"codec_parse_rate", "codec_set_rate"} <= _exported(pkg.CODEC_LIB_PATH)


def _args(h, n_tables=2, depth=8):
    buf = (C.c_uint8 * (16 * 16 * 8 * 3))()
    tabs = (C.c_int32 * (32 * 22))(*([7] * (32 * 22)))
    bits = (C.c_uint64 * (32 * 3))()
    return [h, C.cast(buf, C.c_void_p), 13, 11, 3, 1, C.cast(tabs, C.c_void_p), n_tables, C.cast(bits, C.c_void_p)], (buf, tabs, bits)


def _with(args, i, v):
    b = list(args)
    b[i] = v
    return b


def test_null_context_is_einval(pkg):
    L = pkg.lib()
    args, keep = _args(None)
    assert L.dct3d_rate_frames(*args) == pkg.DCT3D_EINVAL
    assert L.dct3d_rate_frames_dev(*(args + [None])) == pkg.DCT3D_EINVAL
    assert L.dct3d_rate_frames(None, None, 0, 0, 0, 0, None, 0, None) == pkg.DCT3D_EINVAL


def test_bad_arguments_with_a_device(pkg):
    """Every argument error is DCT3D_EINVAL (checked where a context can be made; here the NULL-context test stands)."""
    L = pkg.lib()
    h = C.c_void_p()
    if L.dct3d_ctx_create(0, 8, 8, 8, C.byref(h)) != pkg.DCT3D_OK:
        return
    try:
        E = pkg.DCT3D_EINVAL
        for f, tail in ((L.dct3d_rate_frames, []), (L.dct3d_rate_frames_dev, [None])):
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


def test_pick_quality(pkg):
    pick = pkg.pick_quality
    mono = {1: 900, 2: 700, 4: 500, 8: 300}
    assert pick(mono, 1000) == 1 and pick(mono, 900) == 1 and pick(mono, 899) == 2
    assert pick(mono, 300) == 8 and pick(mono, 499.5) == 8
    assert pick(mono, 299) == 8 and pick(mono, 0) == 8  # none fits: the largest quality
    # no monotonicity assumed: the smallest quality that fits, even when a larger one costs more
    bumpy = {1: 900, 2: 400, 3: 650, 5: 390, 8: 700}
    assert pick(bumpy, 450) == 2 and pick(bumpy, 395) == 5 and pick(bumpy, 650) == 2 and pick(bumpy, 100) == 8
    assert pick({64: 10, 3: 20, 16: 5}, 12) == 16  # the dict's order does not matter
    assert pick({7: 10}, 5) == 7
    with pytest.raises(ValueError):
        pick({}, 5)


def _codec(pkg):
    pkg.lib()
    L = C.CDLL(pkg.CODEC_LIB_PATH)
    L.codec_parse_rate.argtypes = [C.c_char_p, C.POINTER(C.c_double)]
    L.codec_set_rate.argtypes = [C.c_char_p]
    L.codec_set_quant.argtypes = [C.c_char_p]
    return L


def test_codec_parse_rate(pkg):
    L = _codec(pkg)
    v = C.c_double(-7.0)
    assert L.codec_parse_rate(b"rate=1.5", C.byref(v)) == 0 and v.value == 1.5
    assert L.codec_parse_rate(b"rate=2", C.byref(v)) == 0 and v.value == 2.0
    assert L.codec_parse_rate(b"rate=.25", C.byref(v)) == 0 and v.value == 0.25
    for bad in (b"rate=", b"rate=-1", b"rate=abc", b"rate=1.5x", b"rate= 1", b"rate=+1", b"rate=0", b"rate=nan",
                b"rate=inf", b"q=5", b"1.5", b"", None):
        v.value = -7.0
        assert L.codec_parse_rate(bad, C.byref(v)) == 1, bad
        assert v.value == -7.0, bad
    assert L.codec_parse_rate(b"rate=1.5", None) == 1


def test_codec_rejects_quant_together_with_rate(pkg, tmp_path):
    L = _codec(pkg)
    L.encode_ex.argtypes = [C.c_char_p, C.c_char_p] + [C.c_int] * 6
    try:
        assert L.codec_set_quant(b"q=3") == 0
        assert L.codec_set_rate(b"rate=1.5") == 1  # a quantiser is set
        assert L.codec_set_quant(None) == 0
        assert L.codec_set_rate(b"rate=1.5") == 0
        assert L.codec_set_rate(b"rate=" + b"1" * 100) == 1  # too long: nothing changes
    finally:
        L.codec_set_rate(None)
        L.codec_set_quant(None)
    # by the environment: the call itself refuses, before it opens a file or a device
    raw = tmp_path / "in.raw"
    np.zeros(8 * 8 * 8, np.uint8).tofile(raw)
    env = dict(os.environ, DCT3D_CODEC_QUANT="q=3", DCT3D_CODEC_RATE="rate=1.5")
    r = subprocess.run([pkg.CLI_PATH, "encode", str(raw), str(tmp_path / "o.bin"), "8", "8", "8"], env=env,
                       capture_output=True, text=True)
    assert r.returncode == 1 and "exclude each other" in r.stdout and not (tmp_path / "o.bin").exists()
    env = dict(os.environ, DCT3D_CODEC_RATE="rate=abc")
    r = subprocess.run([pkg.CLI_PATH, "encode", str(raw), str(tmp_path / "o.bin"), "8", "8", "8"], env=env,
                       capture_output=True, text=True)
    assert r.returncode == 1 and "Invalid rate target" in r.stdout and not (tmp_path / "o.bin").exists()


@pytest.mark.parametrize("args,said", [
    (["decode", "IN", "OUT", "8", "8", "8", "1", "8", "rate=1.5"], "rate= applies to encode"),
    (["decode_rgb", "IN", "OUT", "8", "8", "8", "1", "8", "rate=1.5"], "rate= applies to encode"),
    (["encode", "IN", "OUT", "8", "8", "8", "1,1", "8", "rate=1.5"], "rate= applies to encode"),
    (["decode", "IN", "OUT", "8", "8", "8", "1,1", "8", "rate=1.5"], "rate= applies to encode"),
    (["encode", "IN", "OUT", "8", "8", "8", "1", "8", "q=3", "rate=1.5"], "exclude each other"),
    (["encode", "IN", "OUT", "8", "8", "8", "1", "8", "rate=1.5", "q=3"], "exclude each other"),
    (["encode_rgb", "IN", "OUT", "8", "8", "8", "1", "4", "rate="], "Invalid rate target"),
    (["encode", "IN", "OUT", "8", "8", "8", "1", "8", "rate=-1"], "Invalid rate target"),
    (["encode", "IN", "OUT", "8", "8", "8", "1", "8", "rate=abc"], "Invalid rate target"),
])
def test_cli_rejects(pkg, tmp_path, args, said):
    """rate= on a decode, with several devices, together with q=, or malformed: refused before any file is made"""
    raw = tmp_path / "in.raw"
    np.zeros(8 * 8 * 8 * 3, np.uint8).tofile(raw)
    out = tmp_path / "out.bin"
    argv = [str(raw) if a == "IN" else str(out) if a == "OUT" else a for a in args]
    r = subprocess.run([pkg.CLI_PATH] + argv, capture_output=True, text=True)
    assert r.returncode == 1 and said in r.stdout, r.stdout
    assert not out.exists() and not (tmp_path / "out.bin.red").exists()


def test_decode_entry_points_reject_a_rate_target(pkg, tmp_path):
    """the library's decode and multi-device entry points refuse a rate target given by the environment"""
    raw = tmp_path / "in.bin"
    np.zeros(64, np.uint8).tofile(raw)
    env = dict(os.environ, DCT3D_CODEC_RATE="rate=1.5")
    for argv in (["decode", str(raw), str(tmp_path / "o.raw"), "8", "8", "8"],
                 ["decode", str(raw), str(tmp_path / "o.raw"), "8", "8", "8", "1,1"],
                 ["encode", str(raw), str(tmp_path / "o.raw"), "8", "8", "8", "1,1"]):
        r = subprocess.run([pkg.CLI_PATH] + argv, env=env, capture_output=True, text=True)
        assert r.returncode == 1 and "rate= applies to single-device encodes only" in r.stdout, r.stdout
        assert not (tmp_path / "o.raw").exists()
