"""CPU: the per-stack quantiser calls (dct3d_*_eg_frames_vq*) are exported, declared and listed and validate their
arguments; the two per-stack pick functions against the scalar rules; the codec's qmap= parser and the CLI's
rejections.  Nothing here needs a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

VQ_SYMBOLS = ("dct3d_encode_eg_frames_vq_dev", "dct3d_encode_eg_frames_vq", "dct3d_decode_eg_frames_vq_dev",
              "dct3d_decode_eg_frames_vq")
LADDER = (1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 24, 32, 40, 48, 64)


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_vq_symbols_exported_declared_and_listed(pkg):
    assert set(VQ_SYMBOLS) <= _exported(pkg.LIB_PATH)
    assert set(VQ_SYMBOLS) <= set(pkg.ABI_SYMBOLS)
    header = open(os.path.join(pkg.INCLUDE_DIR, "dct3d.h")).read()
    for name in VQ_SYMBOLS:
        assert re.search(r"^int %s\(dct3d_ctx \*ctx," % name, header, re.M), name
    assert re.search(r"^#define DCT3D_ABI_VERSION 9$", header, re.M)  # additive: detected by symbol
    assert {"codec_parse_qmap", "codec_set_qmap"} <= _exported(pkg.CODEC_LIB_PATH)
    for name in ("encode_eg_frames_vq", "encode_eg_frames_vq_dev", "decode_eg_frames_vq", "decode_eg_frames_vq_dev"):
        assert callable(getattr(pkg.Context, name))


def _calls(pkg, h, n_tables=2, n_stacks=2):
    """the four calls on 13 x 11 RGB frames, each as (function, argument list, index of tables / n_tables / map)"""
    L = pkg.lib()
    vp = lambda a: C.cast(a, C.c_void_p)
    fr = (C.c_uint8 * (13 * 11 * 3 * 8 * n_stacks))()
    tabs = (C.c_int32 * (33 * 22))(*([7] * (33 * 22)))
    smap = (C.c_uint8 * 8)(*([1] * 8))
    cb, cn = (C.c_uint8 * 3)(), (C.c_int * 3)()
    outs, caps, tb = (C.c_void_p * 3)(), (C.c_uint64 * 3)(), (C.c_uint64 * 3)()
    nb, sb64, sb32, eb = (C.c_uint64 * 3)(64, 64, 64), (C.c_uint64 * 3)(), (C.c_int * 3)(), (C.c_uint64 * 3)()
    streams = (C.c_void_p * 3)(*[C.cast((C.c_uint8 * 64)(), C.c_void_p).value] * 3)
    keep = (fr, tabs, smap, cb, cn, outs, caps, tb, nb, sb64, sb32, eb, streams)
    head = [h, vp(fr), 13, 11, 3, n_stacks, vp(tabs), n_tables, vp(smap)]
    dhead = [13, 11, 3, n_stacks, vp(tabs), n_tables, vp(smap)]
    return [
        (L.dct3d_encode_eg_frames_vq, head + [vp(cb), vp(cn), vp(tb)], (6, 7, 8)),
        (L.dct3d_encode_eg_frames_vq_dev, head + [vp(cb), vp(cn), vp(outs), vp(caps), vp(tb)], (6, 7, 8)),
        (L.dct3d_decode_eg_frames_vq, [h, vp(streams), vp(nb), vp(sb32)] + dhead + [vp(fr), vp(eb)], (8, 9, 10)),
        (L.dct3d_decode_eg_frames_vq_dev, [h, vp(streams), vp(nb), vp(sb64)] + dhead + [vp(fr), vp(eb)], (8, 9, 10)),
    ], keep


def _with(args, i, v):
    b = list(args)
    b[i] = v
    return b


def test_null_context_and_null_arguments_are_einval(pkg):
    calls, keep = _calls(pkg, None)
    for f, args, (it, _, im) in calls:
        assert f(*args) == pkg.DCT3D_EINVAL, f.__name__
        assert f(*_with(args, it, None)) == pkg.DCT3D_EINVAL
        assert f(*_with(args, im, None)) == pkg.DCT3D_EINVAL


def test_bad_arguments_with_a_device(pkg):
    """Every argument error that needs a context is DCT3D_EINVAL (checked where one can be made; without a device
    the NULL-context test stands)."""
    L = pkg.lib()
    h = C.c_void_p()
    if L.dct3d_ctx_create(0, 8, 8, 8, C.byref(h)) != pkg.DCT3D_OK:
        return
    try:
        E = pkg.DCT3D_EINVAL
        calls, keep = _calls(pkg, h)
        for f, args, (it, nt, im) in calls:
            for i, v in ((it, None), (im, None), (nt, 0), (nt, 33), (nt, -1), (nt, 1)):  # (n_tables = 1: the map's 1s)
                assert f(*_with(args, i, v)) == E, (f.__name__, i, v)
        for bad in (0, 256, -3):
            calls, keep = _calls(pkg, h)
            keep[1][22 + 5] = bad  # a step of the second table
            for f, args, _ in calls:
                assert f(*args) == E, (f.__name__, bad)
        calls, keep = _calls(pkg, h)
        keep[2][1] = 2  # the second stack's entry == n_tables
        for f, args, _ in calls:
            assert f(*args) == E, f.__name__
        assert L.dct3d_ctx_set_option(h, pkg.DCT3D_OPT_EG_TWO_STEP, 1.0) == pkg.DCT3D_OK
        calls, keep = _calls(pkg, h)
        for f, args, _ in calls:
            assert f(*args) == E, f.__name__  # the option is refused, not ignored
    finally:
        L.dct3d_ctx_destroy(h)


# ---- the pick functions: the scalar rules, stack by stack -----------------------------------------------------------

def _bumpy(rng, stacks, channels):
    """[T, stacks, channels] sums that are not monotone in the quality"""
    a = rng.integers(0, 5000, size=(len(LADDER), stacks, channels)).astype(np.uint64)
    a[:, 0, :] = 0                      # a stack every quality fits / reaches
    a[:, 1, :] = 2**40                  # a stack no quality fits / reaches
    return a


def test_pick_stack_qualities_is_pick_quality_per_stack(pkg):
    rng = np.random.default_rng(20261020)
    for channels in (1, 3):
        bits = _bumpy(rng, 9, channels)
        assert not all(np.all(np.diff(bits[:, s].sum(axis=1).astype(np.int64)) <= 0) for s in range(2, 9))
        for target in (0, 1, 2500.5, 7000, 2**41):
            got = pkg.pick_stack_qualities(bits, LADDER, target)
            want = [pkg.pick_quality({q: int(bits[t, s].sum()) for t, q in enumerate(LADDER)}, target) for s in range(9)]
            assert got == want and all(isinstance(q, int) for q in got)
        assert pkg.pick_stack_qualities(bits, LADDER, 2500)[:2] == [1, 64]
    with pytest.raises(ValueError):
        pkg.pick_stack_qualities(np.zeros((3, 2, 1)), LADDER, 5)


def test_pick_stack_qualities_psnr_is_pick_quality_psnr_per_stack(pkg):
    rng = np.random.default_rng(20261021)
    for channels in (1, 3):
        sse = _bumpy(rng, 9, channels)
        n = 64 * 64 * 8 * channels
        for db in (1.0, 35.0, 38.5, 200.0):
            got = pkg.pick_stack_qualities_psnr(sse, LADDER, n, db)
            want = [pkg.pick_quality_psnr({q: int(sse[t, s].sum()) for t, q in enumerate(LADDER)}, n, db) for s in range(9)]
            assert got == want
        assert pkg.pick_stack_qualities_psnr(sse, LADDER, n, 60.0)[:2] == [64, 1]
    with pytest.raises(ValueError):
        pkg.pick_stack_qualities_psnr(np.zeros((3, 2, 1)), LADDER, 10, 5)


# ---- the codec's qmap= --------------------------------------------------------------------------------------------

def _codec(pkg):
    pkg.lib()
    L = C.CDLL(pkg.CODEC_LIB_PATH)
    L.codec_parse_qmap.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_int)]
    L.codec_set_qmap.argtypes = [C.c_char_p]
    L.codec_set_quant.argtypes = [C.c_char_p]
    return L


def test_codec_parse_qmap(pkg, tmp_path):
    L = _codec(pkg)
    f = tmp_path / "m.txt"
    out = (C.c_int * 4)(-7, -7, -7, -7)

    def parse(text, n=3):
        f.write_text(text)
        for i in range(4):
            out[i] = -7
        return L.codec_parse_qmap(str(f).encode(), n, out), list(out)

    assert parse("5\n64\n1\n") == (0, [5, 64, 1, -7])
    assert parse("5\n64\n1") == (0, [5, 64, 1, -7])          # no newline after the last line
    assert parse("12\r\n12\r\n12\r\n") == (0, [12, 12, 12, -7])
    for bad in ("5\n64\n", "5\n64\n1\n2\n",                   # another line count
                "5\n7\n1\n", "5\n0\n1\n", "5\n65\n1\n", "5\n255\n1\n",  # no quality of the ladder
                "", "\n", "5\n\n1\n", "5\n 6\n1\n", "5\n6 \n1\n", "5\n+6\n1\n", "5\n-6\n1\n", "5\n6.0\n1\n", "5,6,1\n", "q=5\n6\n1\n"):
        assert parse(bad) == (1, [-7] * 4), repr(bad)
    assert L.codec_parse_qmap(str(tmp_path / "missing.txt").encode(), 3, out) == 1
    f.write_text("5\n64\n1\n")
    assert L.codec_parse_qmap(None, 3, out) == 1 and L.codec_parse_qmap(str(f).encode(), 0, out) == 1
    assert L.codec_parse_qmap(str(f).encode(), 3, None) == 1


def test_codec_set_qmap_and_a_quantiser_exclude_each_other(pkg):
    L = _codec(pkg)
    try:
        assert L.codec_set_quant(b"q=3") == 0
        assert L.codec_set_qmap(b"qmap=/tmp/x") == 1
        assert L.codec_set_quant(None) == 0
        assert L.codec_set_qmap(b"qmap=/tmp/x") == 0
        assert L.codec_set_qmap(b"qmap=" + b"x" * 5000) == 1  # too long: nothing changes
    finally:
        L.codec_set_qmap(None)
        L.codec_set_quant(None)


@pytest.mark.parametrize("args,env,said", [
    (["encode", "IN", "OUT", "8", "8", "16", "1", "8", "q=3", "qmap=MAP"], {}, "exclude each other"),
    (["encode", "IN", "OUT", "8", "8", "16", "1", "8", "qmap=MAP", "q=3"], {}, "exclude each other"),
    (["decode", "IN", "OUT", "8", "8", "16", "1", "8", "q=3", "qmap=MAP"], {}, "exclude each other"),
    (["encode", "IN", "OUT", "8", "8", "16", "1,1", "8", "qmap=MAP"], {}, "one device"),
    (["decode", "IN", "OUT", "8", "8", "16", "1,1", "8", "qmap=MAP"], {}, "one device"),
    (["encode_rgb", "IN", "OUT", "8", "8", "16", "1", "8", "qmap="], {}, "Invalid quality map"),
    (["encode", "IN", "OUT", "8", "8", "16", "1", "8"], {"DCT3D_CODEC_QMAP": "qmap=MAP", "DCT3D_CODEC_QUANT": "q=3"},
     "exclude each other"),
    (["encode", "IN", "OUT", "8", "8", "16", "1,1", "8"], {"DCT3D_CODEC_QMAP": "qmap=MAP"}, "single-device"),
    (["decode", "IN", "OUT", "8", "8", "16", "1,1", "8"], {"DCT3D_CODEC_QMAP": "qmap=MAP"}, "single-device"),
    (["encode", "IN", "OUT", "8", "8", "16", "1", "8", "qmap=MAP"], {"DCT3D_CODEC_HOST_EG": "1"}, "DCT3D_CODEC_HOST_EG"),
    (["encode", "IN", "OUT", "8", "8", "24", "1", "8", "qmap=MAP"], {}, "Invalid quality map file"),   # 3 stacks, 2 lines
    (["decode", "IN", "OUT", "8", "8", "24", "1", "8", "qmap=MAP"], {}, "Invalid quality map file"),
    (["decode_rgb", "IN", "OUT", "8", "8", "16", "1", "8", "qmap=BAD"], {}, "Invalid quality map file"),  # a 7
    (["encode", "IN", "OUT", "8", "8", "16", "1", "8", "qmap=MISSING"], {}, "Invalid quality map file"),
])
def test_cli_rejects(pkg, tmp_path, args, env, said):
    """qmap= with q=, with several devices, on the host Exp-Golomb path, or with a bad map file: refused before any
    output file is made (and before a device is needed)"""
    raw, out, good, bad = tmp_path / "in.raw", tmp_path / "out.bin", tmp_path / "map.txt", tmp_path / "bad.txt"
    np.zeros(8 * 8 * 24 * 3, np.uint8).tofile(raw)
    good.write_text("5\n12\n")
    bad.write_text("5\n7\n")
    names = {"IN": str(raw), "OUT": str(out), "qmap=MAP": "qmap=" + str(good), "qmap=BAD": "qmap=" + str(bad),
             "qmap=MISSING": "qmap=" + str(tmp_path / "none.txt")}
    argv = [names.get(a, a) for a in args]
    env = {k: names.get(v, v) for k, v in env.items()}
    r = subprocess.run([pkg.CLI_PATH] + argv, capture_output=True, text=True, env=dict(os.environ, **env))
    assert r.returncode == 1 and said in r.stdout, r.stdout
    assert not out.exists() and not (tmp_path / "out.bin.red").exists()
    assert good.read_text() == "5\n12\n"
