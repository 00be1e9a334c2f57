"""CPU: the RGB-domain distortion probe's entry points (dct3d_distortion_rgb_frames*) are exported,
declared and listed and validate their arguments; pick_stack_channel_qualities_psnr against a brute-force
restatement; the codec's psnr_rgb= parser, its exclusions and the CLI's rejections; the old refusal texts of psnr=
with ycc=1.  One test, marked gpu, needs a device: the argument errors behind the context check."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

RGB_SYMBOLS = ("dct3d_distortion_rgb_frames_dev", "dct3d_distortion_rgb_frames")
CODEC_SYMBOLS = ("codec_parse_psnr_rgb", "codec_set_psnr_rgb")


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_symbols_exported_declared_and_listed(pkg):
    assert set(RGB_SYMBOLS) <= _exported(pkg.LIB_PATH)
    assert set(RGB_SYMBOLS) <= set(pkg.ABI_SYMBOLS)
    header = open(os.path.join(pkg.INCLUDE_DIR, "dct3d.h")).read()
    for name in RGB_SYMBOLS:
        assert re.search(r"^int %s\(dct3d_ctx \*ctx," % name, header, re.M), name
    assert re.search(r"^#define DCT3D_RGB_PLANE_BUDGET \(64u << 20\)$", header, re.M) and pkg.DCT3D_RGB_PLANE_BUDGET == 64 << 20
    assert set(CODEC_SYMBOLS) <= _exported(pkg.CODEC_LIB_PATH)
    codec_h = open(os.path.join(pkg.INCLUDE_DIR, "codec.h")).read()
    for name in CODEC_SYMBOLS:
        assert re.search(r"^int %s\(const char \*text" % name, codec_h, re.M), name
    assert hasattr(pkg.Context, "distortion_rgb_frames") and hasattr(pkg.Context, "distortion_rgb_frames_dev")


def _args(h, n_tables=2, n_cand=2):
    """[ctx, frames, w, h, n_stacks, tables, n_tables, cand, n_cand, sse, plane_sse, bits]"""
    buf = (C.c_uint8 * (16 * 16 * 8 * 3))()
    tabs = (C.c_int32 * (32 * 22))(*([7] * (32 * 22)))
    cand = (C.c_uint8 * (3 * 33))(*([0, 1, 0] * 33))
    sse = (C.c_uint64 * 64)()
    planes = (C.c_uint64 * (32 * 3))()
    bits = (C.c_uint64 * (32 * 3))()
    vp = C.c_void_p
    return [h, C.cast(buf, vp), 13, 11, 1, C.cast(tabs, vp), n_tables, C.cast(cand, vp), n_cand, C.cast(sse, vp),
            C.cast(planes, vp), C.cast(bits, vp)], (buf, tabs, cand, sse, planes, bits)


def _with(args, i, v):
    b = list(args)
    b[i] = v
    return b


def test_null_context_is_einval(pkg):
    L = pkg.lib()
    args, keep = _args(None)
    assert L.dct3d_distortion_rgb_frames(*args) == pkg.DCT3D_EINVAL
    assert L.dct3d_distortion_rgb_frames_dev(*(args + [None])) == pkg.DCT3D_EINVAL
    assert L.dct3d_distortion_rgb_frames(None, None, 0, 0, 0, None, 0, None, 0, None, None, None) == pkg.DCT3D_EINVAL
    # every bad argument of the list below, on a NULL context: still DCT3D_EINVAL, nothing is dereferenced
    for i, v in ((2, 0), (4, -1), (1, None), (9, None), (6, 0), (6, 33), (8, 0), (8, 33)):
        assert L.dct3d_distortion_rgb_frames(*_with(args, i, v)) == pkg.DCT3D_EINVAL
        assert L.dct3d_distortion_rgb_frames_dev(*(_with(args, i, v) + [None])) == pkg.DCT3D_EINVAL


@pytest.mark.gpu
def test_bad_arguments_with_a_device(pkg):
    """Every argument error that needs a context is DCT3D_EINVAL, through the C-ABI itself (the one test of this module
    that needs a device); the same arguments without the error are accepted, with plane_sse == NULL and bits == NULL
    too."""
    L = pkg.lib()
    h = C.c_void_p()
    assert L.dct3d_ctx_create(0, 8, 8, 8, C.byref(h)) == pkg.DCT3D_OK
    try:
        E = pkg.DCT3D_EINVAL
        # (the host-pointer call alone: the frames of _args are host memory)
        args, keep = _args(h)
        assert L.dct3d_distortion_rgb_frames(*args) == pkg.DCT3D_OK  # the arguments every case below spoils
        assert L.dct3d_distortion_rgb_frames(*_with(_with(args, 10, None), 11, None)) == pkg.DCT3D_OK
        for f, tail in ((L.dct3d_distortion_rgb_frames, []), (L.dct3d_distortion_rgb_frames_dev, [None])):
            args, keep = _args(h)
            # what the rate probe's check refuses; sse == NULL; n_cand outside 1..32
            for i, v in ((2, 0), (3, -1), (4, -1), (1, None), (9, None), (6, 0), (6, 33), (6, -1), (8, 0), (8, 33), (8, -1)):
                assert f(*(_with(args, i, v) + tail)) == E, (f.__name__, i, v)
            assert f(*(_with(_with(args, 5, None), 6, 2) + tail)) == E  # tables == NULL needs n_tables == 1
            assert f(*(_with(_with(args, 7, None), 8, 3) + tail)) == E  # cand == NULL needs n_cand == n_tables
            for bad in (0, 256, -3):
                args, keep = _args(h)
                keep[1][22 + 5] = bad  # a step of the second table
                assert f(*(args + tail)) == E, bad
            args, keep = _args(h)
            keep[2][4] = 2  # a candidate index >= n_tables
            assert f(*(args + tail)) == E
            # 4:2:0 without the colour transform
            args, keep = _args(h)
            assert L.dct3d_ctx_set_chroma(h, pkg.DCT3D_CHROMA_420) == pkg.DCT3D_OK
            try:
                assert f(*(args + tail)) == E
            finally:
                L.dct3d_ctx_set_chroma(h, pkg.DCT3D_CHROMA_444)
    finally:
        L.dct3d_ctx_destroy(h)


def test_context_methods_refuse_wrong_shapes_before_the_library(pkg):
    """grey frames and a malformed candidate list never reach the library (no context needed to see it)"""
    ctx = object.__new__(pkg.Context)
    ctx._h, ctx.bw, ctx.bh, ctx.bd = None, 8, 8, 8
    try:
        with pytest.raises(pkg.Dct3dError) as e:
            ctx.distortion_rgb_frames(np.zeros((8, 8, 8), np.uint8))
        assert e.value.code == pkg.DCT3D_EINVAL
        for bad in ([(0, 0)], [[0, 0, 256]], [[0, -1, 0]], []):
            with pytest.raises(pkg.Dct3dError) as e:
                ctx.distortion_rgb_frames(np.zeros((8, 8, 8, 3), np.uint8), None, bad)
            assert e.value.code == pkg.DCT3D_EINVAL
    finally:
        ctx._h = None


def _brute(pkg, sse, qualities, n, target, rungs):
    """the rule restated: per stack, over the candidates (q_i, q_j, q_j), the largest q_i whose PSNR reaches the
    target; else the smallest q_i"""
    T = len(qualities)
    res = []
    for s in range(sse.shape[1]):
        ok = [qualities[i] for i in range(T) if pkg.psnr_db(int(sse[i, s]), n) >= target]
        q = max(ok) if ok else min(qualities)
        i = qualities.index(q)
        j = min(i + rungs, T - 1)
        res.append((q, qualities[j], qualities[j]))
    return res


def test_pick_stack_channel_qualities_psnr(pkg):
    pick = pkg.pick_stack_channel_qualities_psnr
    n = 3 * 61 * 45 * 8
    at = lambda db: int(round(255 * 255 * n / 10 ** (db / 10)))  # noqa: E731
    q = [1, 2, 4, 8, 16]
    mono = np.array([[at(45), at(44)], [at(40), at(41)], [at(35), at(36)], [at(30), at(29)], [at(25), at(20)]], np.uint64)
    assert pick(mono, q, n, 32) == [(4, 4, 4), (4, 4, 4)]
    assert pick(mono, q, n, 32, 2) == [(4, 16, 16), (4, 16, 16)]
    assert pick(mono, q, n, 29.5, 1) == [(8, 16, 16), (4, 8, 8)]
    assert pick(mono, q, n, 99) == [(1, 1, 1), (1, 1, 1)]  # none reaches it: the smallest
    assert pick(mono, q, n, 1, 3) == [(16, 16, 16), (16, 16, 16)]  # j is clipped to the last rung
    # non-monotone errors, every target between the rungs, every offset: the brute-force restatement
    rng = np.random.default_rng(20261020)
    for trial in range(20):
        T = int(rng.integers(1, 7))
        quals = sorted(rng.choice(np.arange(1, 65), T, replace=False).tolist())
        if trial % 3 == 0:
            quals = quals[::-1]  # the order of the list does not matter to the rule
        sse = rng.integers(0, 3, (T, 4)) * rng.integers(1, 10**9, (T, 4))
        for target, rungs in itertools.product((5.0, 20.0, 33.3, 48.0, 1e9), (0, 1, 2, 7)):
            assert pick(sse, quals, n, target, rungs) == _brute(pkg, sse, quals, n, target, rungs)
    assert pick(np.array([[0], [at(30)], [0]]), [1, 2, 3], n, 1e9) == [(3, 3, 3)]  # sse == 0 reaches every target
    for bad in (lambda: pick(mono[:4], q, n, 30), lambda: pick(mono[..., None], q, n, 30), lambda: pick(mono, q, n, 30, -1),
                lambda: pick(mono, q, n, 30, 0.5)):
        with pytest.raises(ValueError):
            bad()


def _codec(pkg):
    pkg.lib()
    L = C.CDLL(pkg.CODEC_LIB_PATH)
    for f in (L.codec_parse_psnr_rgb, L.codec_parse_psnr, L.codec_parse_rate):
        f.argtypes = [C.c_char_p, C.POINTER(C.c_double)]
    for f in (L.codec_set_psnr_rgb, L.codec_set_psnr, L.codec_set_rate, L.codec_set_quant):
        f.argtypes = [C.c_char_p]
    return L


def test_codec_parse_psnr_rgb(pkg):
    L = _codec(pkg)
    v = C.c_double(-7.0)
    assert L.codec_parse_psnr_rgb(b"psnr_rgb=38.5", C.byref(v)) == 0 and v.value == 38.5
    assert L.codec_parse_psnr_rgb(b"psnr_rgb=40", C.byref(v)) == 0 and v.value == 40.0
    assert L.codec_parse_psnr_rgb(b"psnr_rgb=.25", C.byref(v)) == 0 and v.value == 0.25
    for tail in ("", "-1", "abc", "1.5x", " 1", "+1", "0", "nan", "inf", "1e2", "0x10"):
        v.value = -7.0
        assert L.codec_parse_psnr_rgb(("psnr_rgb=" + tail).encode(), C.byref(v)) == 1, tail
        assert v.value == -7.0, tail
    for bad in (b"q=5", b"psnr=38.5", b"rate=1.5", b"38.5", b"", None):
        v.value = -7.0
        assert L.codec_parse_psnr_rgb(bad, C.byref(v)) == 1, bad
        assert v.value == -7.0, bad
    assert L.codec_parse_psnr_rgb(b"psnr_rgb=38.5", None) == 1
    # the plane-domain parser does not take the new text
    assert L.codec_parse_psnr(b"psnr_rgb=38.5", C.byref(v)) == 1


def test_codec_set_psnr_rgb_is_exclusive(pkg, tmp_path):
    L = _codec(pkg)
    try:
        for other, text in ((L.codec_set_quant, b"q=3"), (L.codec_set_rate, b"rate=1.5"), (L.codec_set_psnr, b"psnr=38")):
            assert other(text) == 0
            assert L.codec_set_psnr_rgb(b"psnr_rgb=38") == 1, text  # another selector is set
            assert other(None) == 0
        assert L.codec_set_psnr_rgb(b"psnr_rgb=38") == 0
        assert L.codec_set_rate(b"rate=1.5") == 1 and L.codec_set_psnr(b"psnr=38") == 1  # the RGB target is set
        assert L.codec_set_psnr_rgb(b"psnr_rgb=" + b"1" * 100) == 1  # too long: nothing changes
        assert L.codec_set_psnr(b"psnr=38") == 1
        assert L.codec_set_psnr_rgb(b"") == 0
        assert L.codec_set_psnr(b"psnr=38") == 0
    finally:
        for f in (L.codec_set_psnr_rgb, L.codec_set_psnr, L.codec_set_rate, L.codec_set_quant):
            f(None)
    # by the environment: the call itself refuses, before it opens a file or a device
    raw = tmp_path / "in.raw"
    np.zeros(8 * 8 * 8 * 3, np.uint8).tofile(raw)
    rgb = [pkg.CLI_PATH, "encode_rgb", str(raw), str(tmp_path / "o"), "8", "8", "8"]
    grey = [pkg.CLI_PATH, "encode", str(raw), str(tmp_path / "o"), "8", "8", "8"]
    for argv, extra, said in ((rgb, {"DCT3D_CODEC_QUANT": "q=3"}, "exclude each other"),
                              (rgb, {"DCT3D_CODEC_RATE": "rate=1.5"}, "exclude each other"),
                              (rgb, {"DCT3D_CODEC_PSNR": "psnr=38"}, "exclude each other"),
                              (rgb, {"DCT3D_CODEC_PSNR_RGB": "psnr_rgb=abc"}, "Invalid psnr_rgb target"),
                              (rgb, {"DCT3D_CODEC_HOST_EG": "1"}, "psnr_rgb= needs the device stream calls"),
                              (grey, {}, "psnr_rgb= applies to encode_rgb")):
        env = dict(os.environ, DCT3D_CODEC_PSNR_RGB="psnr_rgb=38")
        env.update(extra)
        r = subprocess.run(argv, env=env, capture_output=True, text=True)
        assert r.returncode == 1 and said in r.stdout, r.stdout
        assert not any(p.name.startswith("o") for p in tmp_path.iterdir()), r.stdout


ONE = ["8", "8", "8", "1", "8"]


@pytest.mark.parametrize("args,said", [
    (["decode_rgb", "IN", "OUT"] + ONE + ["psnr_rgb=38"], "psnr_rgb= applies to encode_rgb on one device"),
    (["decode", "IN", "OUT"] + ONE + ["psnr_rgb=38"], "psnr_rgb= applies to encode_rgb on one device"),
    (["encode", "IN", "OUT"] + ONE + ["psnr_rgb=38"], "psnr_rgb= applies to encode_rgb on one device"),
    (["encode_rgb", "IN", "OUT", "8", "8", "8", "1,1", "8", "psnr_rgb=38"], "psnr_rgb= applies to encode_rgb on one device"),
    (["encode_rgb", "IN", "OUT"] + ONE + ["q=3", "psnr_rgb=38"], "q= and psnr_rgb= exclude each other"),
    (["encode_rgb", "IN", "OUT"] + ONE + ["psnr_rgb=38", "q=3"], "q= and psnr_rgb= exclude each other"),
    (["encode_rgb", "IN", "OUT"] + ONE + ["rate=1.5", "psnr_rgb=38"], "rate= and psnr_rgb= exclude each other"),
    (["encode_rgb", "IN", "OUT"] + ONE + ["psnr_rgb=38", "psnr=38"], "psnr= and psnr_rgb= exclude each other"),
    (["encode_rgb", "IN", "OUT"] + ONE + ["psnr_rgb="], "Invalid psnr_rgb target"),
    (["encode_rgb", "IN", "OUT"] + ONE + ["psnr_rgb=-1"], "Invalid psnr_rgb target"),
    (["encode_rgb", "IN", "OUT"] + ONE + ["psnr_rgb=abc"], "Invalid psnr_rgb target"),
    (["encode_rgb", "IN", "OUT"] + ONE + ["psnr_rgb=38", "ycc=1", "qmap=MAP", "cq=1"], "cq= applies to an encode_rgb with"),
    (["encode_rgb", "IN", "OUT"] + ONE + ["psnr_rgb=38", "ycc=1", "cq=1"], "cq= applies to an encode_rgb with"),
    (["encode_rgb", "IN", "OUT"] + ONE + ["psnr_rgb=38", "qmap3=MAP", "cq=1"], "cq= needs ycc=1"),
    (["encode_rgb", "IN", "OUT"] + ONE + ["psnr_rgb=38", "chroma=420"], "chroma=420 needs ycc=1"),
    # the old refusals of the plane-domain target, word for word
    (["encode_rgb", "IN", "OUT"] + ONE + ["psnr=38", "ycc=1"],
     "ycc=1 and psnr= exclude each other: the distortion probe would measure the Y, Cb, Cr planes, not the RGB samples"),
    (["encode_rgb", "IN", "OUT"] + ONE + ["psnr=38", "qmap3=MAP"], "qmap3= excludes q=, qmap= and psnr="),
])
def test_cli_rejects(pkg, tmp_path, args, said):
    """psnr_rgb= on a decode, on a grey command, with several devices, together with q=, rate= or psnr=, malformed,
    or with a cq= that has no three-column map: refused before any file is made"""
    raw = tmp_path / "in.raw"
    np.zeros(8 * 8 * 8 * 3, np.uint8).tofile(raw)
    out = tmp_path / "out.bin"
    argv = [str(raw) if a == "IN" else str(out) if a == "OUT" else a.replace("MAP", str(tmp_path / "map.txt")) for a in args]
    r = subprocess.run([pkg.CLI_PATH] + argv, capture_output=True, text=True)
    assert r.returncode == 1 and said in r.stdout, r.stdout
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.raw"], r.stdout


def test_the_old_psnr_refusal_by_the_library(pkg, tmp_path):
    """ycc=1 by the environment beside psnr=: the library's own message is the old one"""
    raw = tmp_path / "in.raw"
    np.zeros(8 * 8 * 8 * 3, np.uint8).tofile(raw)
    env = dict(os.environ, DCT3D_CODEC_YCC="1")
    r = subprocess.run([pkg.CLI_PATH, "encode_rgb", str(raw), str(tmp_path / "o"), "8", "8", "8", "1", "8", "psnr=38"],
                       env=env, capture_output=True, text=True)
    assert r.returncode == 1, r.stdout
    assert "ycc=1 and psnr= exclude each other: the distortion probe would measure the Y, Cb, Cr planes, not the RGB samples" \
        in r.stdout.replace("\n", " ").replace("the  RGB", "the RGB")
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.raw"]


def test_decode_entry_points_reject_the_target(pkg, tmp_path):
    """the library's decode and multi-device entry points refuse the target given by the environment"""
    raw = tmp_path / "in.bin"
    np.zeros(64, np.uint8).tofile(raw)
    env = dict(os.environ, DCT3D_CODEC_PSNR_RGB="psnr_rgb=38")
    for argv in (["decode", str(raw), str(tmp_path / "o.raw"), "8", "8", "8"],
                 ["decode_rgb", str(raw), str(tmp_path / "o.raw"), "8", "8", "8"],
                 ["decode", str(raw), str(tmp_path / "o.raw"), "8", "8", "8", "1,1"],
                 ["encode", str(raw), str(tmp_path / "o.raw"), "8", "8", "8", "1,1"]):
        r = subprocess.run([pkg.CLI_PATH] + argv, env=env, capture_output=True, text=True)
        assert r.returncode == 1 and "psnr_rgb= applies to single-device encodes only" in r.stdout, (argv, r.stdout)
        assert not (tmp_path / "o.raw").exists()
