"""CPU: the SSIM probe's entry points (dct3d_ssim_frames*, dct3d_ssim_windows) are exported, declared and listed and
validate their arguments; ssim_mean and the pick rules; the codec's ssim= parser and the CLI's rejections.  Only the
argument errors behind a live context need a device (marked gpu)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

SSIM_SYMBOLS = ("dct3d_ssim_frames_dev", "dct3d_ssim_frames", "dct3d_ssim_windows")
ONE = 1 << 24


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_ssim_symbols_exported_declared_and_listed(pkg):
    assert set(SSIM_SYMBOLS) <= _exported(pkg.LIB_PATH)
    assert set(SSIM_SYMBOLS) <= set(pkg.ABI_SYMBOLS)
    header = open(os.path.join(pkg.INCLUDE_DIR, "dct3d.h")).read()
    for name in SSIM_SYMBOLS[:2]:
        assert re.search(r"^int %s\(dct3d_ctx \*ctx," % name, header, re.M), name
    assert re.search(r"^int dct3d_ssim_windows\(int w, int h, int \*nwx, int \*nwy\);", header, re.M)
    m = re.search(r"^#define DCT3D_SSIM_BLOCK_BUDGET \((\d+)u << (\d+)\)", header, re.M)
    assert m and int(m.group(1)) << int(m.group(2)) == pkg.DCT3D_SSIM_BLOCK_BUDGET
    # the budget's own requirement: 32 tables at 256 x 176 overflow it with 2 .. 8 stacks, at both depths
    for depth in (8, 4):
        per_stack = depth * (256 // 4) * (176 // 4) * (8 * 32 + 4)
        assert 2 <= pkg.DCT3D_SSIM_BLOCK_BUDGET // per_stack + 1 <= 8, depth
    assert {"codec_parse_ssim", "codec_set_ssim"} <= _exported(pkg.CODEC_LIB_PATH)
    codec_h = open(os.path.join(pkg.INCLUDE_DIR, "codec.h")).read()
    for name in ("codec_parse_ssim", "codec_set_ssim"):
        assert re.search(r"^int %s\(const char \*text" % name, codec_h, re.M), name


def test_ssim_windows(pkg):
    assert pkg.ssim_windows(1, 1) == (1, 1) and pkg.ssim_windows(4, 4) == (1, 1) and pkg.ssim_windows(5, 3) == (1, 1)
    assert pkg.ssim_windows(8, 8) == (1, 1) and pkg.ssim_windows(9, 4) == (2, 1) and pkg.ssim_windows(61, 45) == (15, 11)
    assert pkg.ssim_windows(64, 64) == (15, 15) and pkg.ssim_windows(1920, 1080) == (479, 269)
    L = pkg.lib()
    a, b = C.c_int(-5), C.c_int(-5)
    for w, h in ((0, 8), (8, 0), (-1, 8), (8, -3), (0, 0)):
        assert L.dct3d_ssim_windows(w, h, C.byref(a), C.byref(b)) == pkg.DCT3D_EINVAL
        assert (a.value, b.value) == (-5, -5)
        with pytest.raises(pkg.Dct3dError):
            pkg.ssim_windows(w, h)
    assert L.dct3d_ssim_windows(8, 8, None, C.byref(b)) == pkg.DCT3D_EINVAL
    assert L.dct3d_ssim_windows(8, 8, C.byref(a), None) == pkg.DCT3D_EINVAL


def _args(h, n_tables=2):
    buf = (C.c_uint8 * (16 * 16 * 8 * 3))()
    tabs = (C.c_int32 * (32 * 22))(*([7] * (32 * 22)))
    ssim = (C.c_int64 * (32 * 3))()
    sse = (C.c_uint64 * (32 * 3))()
    bits = (C.c_uint64 * (32 * 3))()
    return [h, C.cast(buf, C.c_void_p), 13, 11, 3, 1, C.cast(tabs, C.c_void_p), n_tables, C.cast(ssim, C.c_void_p),
            C.cast(sse, C.c_void_p), C.cast(bits, C.c_void_p)], (buf, tabs, ssim, sse, bits)


def _with(args, i, v):
    b = list(args)
    b[i] = v
    return b


def test_null_context_is_einval(pkg):
    L = pkg.lib()
    args, keep = _args(None)
    assert L.dct3d_ssim_frames(*args) == pkg.DCT3D_EINVAL
    assert L.dct3d_ssim_frames_dev(*(args + [None])) == pkg.DCT3D_EINVAL
    assert L.dct3d_ssim_frames(None, None, 0, 0, 0, 0, None, 0, None, None, None) == pkg.DCT3D_EINVAL


@pytest.mark.gpu
def test_bad_arguments_with_a_device(pkg):
    """Every argument error is DCT3D_EINVAL, and nothing but the spoiled argument makes it one: the unspoiled
    arguments return DCT3D_OK, with sse == NULL and bits == NULL too.  (rate_args_ok looks at the context first, so a
    context is needed: the host-pointer call takes these arguments as they are; the device call takes the frames from
    a device buffer.)"""
    import torch
    L = pkg.lib()
    h = C.c_void_p()
    assert L.dct3d_ctx_create(0, 8, 8, 8, C.byref(h)) == pkg.DCT3D_OK
    d_fr = torch.zeros(16 * 16 * 8 * 3, dtype=torch.uint8, device="cuda")
    try:
        E = pkg.DCT3D_EINVAL
        for f, tail, frames in ((L.dct3d_ssim_frames, [], None), (L.dct3d_ssim_frames_dev, [None], d_fr.data_ptr())):
            args, keep = _args(h)
            if frames is not None:
                args[1] = frames
            for n_tables in (2, 1, 32):
                assert f(*(_with(args, 7, n_tables) + tail)) == pkg.DCT3D_OK, (f.__name__, n_tables)
            assert f(*(_with(args, 9, None) + tail)) == pkg.DCT3D_OK      # sse == NULL
            assert f(*(_with(args, 10, None) + tail)) == pkg.DCT3D_OK     # bits == NULL
            assert f(*(_with(_with(args, 9, None), 10, None) + tail)) == pkg.DCT3D_OK
            assert f(*(_with(_with(args, 6, None), 7, 1) + tail)) == pkg.DCT3D_OK  # the context's table
            assert keep[2][0] > 0  # (13 x 11 zeros: every window is 1)
            for i, v in ((2, 0), (3, -1), (4, 2), (4, 0), (5, -1), (1, None), (8, None), (7, 0), (7, 33), (7, -1)):
                assert f(*(_with(args, i, v) + tail)) == E, (f.__name__, i, v)
            assert f(*(_with(_with(args, 6, None), 7, 2) + tail)) == E  # tables == NULL needs n_tables == 1
            for bad in (0, 256, -3):
                args, keep = _args(h)
                keep[1][22 + 5] = bad  # a step of the second table
                assert f(*(args + tail)) == E, bad
    finally:
        L.dct3d_ctx_destroy(h)


def test_pick_quality_ssim(pkg):
    pick = pkg.pick_quality_ssim
    n = 1000
    tot = lambda s: int(round(s * ONE * n))  # noqa: E731
    mono = {1: tot(0.99), 2: tot(0.95), 4: tot(0.90), 8: tot(0.80)}
    assert pick(mono, n, 0.7) == 8 and pick(mono, n, 0.85) == 4 and pick(mono, n, 0.93) == 2 and pick(mono, n, 0.97) == 1
    assert pick(mono, n, 0.999) == 1  # none reaches the target: the smallest quality
    assert pick(mono, n, pkg.ssim_mean(mono[4], n)) == 4  # >=: a quality exactly at the target counts
    # no monotonicity assumed: the largest quality that reaches the target, even when a smaller one does not
    bumpy = {1: tot(0.95), 2: tot(0.60), 3: tot(0.85), 5: tot(0.50), 8: tot(0.70)}
    assert pick(bumpy, n, 0.65) == 8 and pick(bumpy, n, 0.8) == 3 and pick(bumpy, n, 0.9) == 1 and pick(bumpy, n, 0.55) == 8
    assert pick(bumpy, n, 1.0) == 1
    assert pick({64: tot(0.2), 3: tot(0.6), 16: tot(0.4)}, n, 0.3) == 16  # the dict's order does not matter
    assert pick({7: tot(0.3)}, n, 0.9) == 7
    assert pick({1: tot(-0.2), 2: tot(-0.5)}, n, 0.1) == 1  # negative means reach nothing
    assert pick({1: ONE * n, 2: tot(0.5), 4: ONE * n}, n, 1.0) == 4  # a mean of exactly 1 reaches the target 1
    with pytest.raises(ValueError):
        pick({}, n, 0.5)


def test_pick_stack_qualities_ssim(pkg):
    n = 100  # windows per stack, both channels together
    tot = lambda s: int(round(s * ONE * n / 2))  # noqa: E731  (per channel)
    qualities = [1, 4, 9, 16]
    #                    stack 0: monotone        stack 1: bumpy           stack 2: nothing reaches it
    per_stack = np.array([[0.99, 0.9, 0.8, 0.7], [0.9, 0.5, 0.85, 0.4], [0.3, 0.2, 0.35, 0.1]])
    ssim = np.empty((4, 3, 2), np.int64)
    for t in range(4):
        for s in range(3):
            ssim[t, s] = (tot(per_stack[s, t] + 0.05), tot(per_stack[s, t] - 0.05))  # the channels add up
    assert pkg.pick_stack_qualities_ssim(ssim, qualities, n, 0.75) == [9, 9, 1]
    assert pkg.pick_stack_qualities_ssim(ssim, qualities, n, 0.3) == [16, 16, 9]
    assert pkg.pick_stack_qualities_ssim(ssim, qualities, n, 0.95) == [1, 1, 1]
    with pytest.raises(ValueError):
        pkg.pick_stack_qualities_ssim(ssim[:3], qualities, n, 0.5)
    with pytest.raises(ValueError):
        pkg.pick_stack_qualities_ssim(ssim[:, :, 0], qualities, n, 0.5)


def _codec(pkg):
    pkg.lib()
    L = C.CDLL(pkg.CODEC_LIB_PATH)
    L.codec_parse_ssim.argtypes = [C.c_char_p, C.POINTER(C.c_double)]
    for f in (L.codec_set_ssim, L.codec_set_psnr, L.codec_set_psnr_rgb, L.codec_set_rate, L.codec_set_quant):
        f.argtypes = [C.c_char_p]
    return L


def test_codec_parse_ssim(pkg):
    L = _codec(pkg)
    v = C.c_double(-7.0)
    assert L.codec_parse_ssim(b"ssim=0.95", C.byref(v)) == 0 and v.value == 0.95
    assert L.codec_parse_ssim(b"ssim=1", C.byref(v)) == 0 and v.value == 1.0
    assert L.codec_parse_ssim(b"ssim=1.0", C.byref(v)) == 0 and v.value == 1.0
    assert L.codec_parse_ssim(b"ssim=.25", C.byref(v)) == 0 and v.value == 0.25
    for tail in ("", "-1", "abc", "0.5x", " 0.5", "+0.5", "0", "0.0", "nan", "inf", "1e-2", "0x1", "1.0001", "2", "38.5"):
        v.value = -7.0
        assert L.codec_parse_ssim(("ssim=" + tail).encode(), C.byref(v)) == 1, tail
        assert v.value == -7.0, tail
    for bad in (b"q=5", b"psnr=0.5", b"0.5", b"", None):
        v.value = -7.0
        assert L.codec_parse_ssim(bad, C.byref(v)) == 1, bad
        assert v.value == -7.0, bad
    assert L.codec_parse_ssim(b"ssim=0.5", None) == 1


def test_codec_set_ssim_is_exclusive_with_the_other_selectors(pkg, tmp_path):
    L = _codec(pkg)
    others = ((L.codec_set_quant, b"q=3"), (L.codec_set_rate, b"rate=1.5"), (L.codec_set_psnr, b"psnr=38"),
              (L.codec_set_psnr_rgb, b"psnr_rgb=38"))
    try:
        for setter, text in others:
            assert setter(text) == 0
            assert L.codec_set_ssim(b"ssim=0.9") == 1, text  # another selector is set
            assert setter(None) == 0
        assert L.codec_set_ssim(b"ssim=0.9") == 0
        for setter, text in others[1:]:
            assert setter(text) == 1, text  # an SSIM target is set
        assert L.codec_set_ssim(b"ssim=" + b"1" * 100) == 1  # too long: nothing changes
        assert L.codec_set_rate(b"rate=1.5") == 1
        assert L.codec_set_ssim(b"") == 0
        assert L.codec_set_rate(b"rate=1.5") == 0
    finally:
        for setter, _ in others:
            setter(None)
        L.codec_set_ssim(None)
    # by the environment: the call itself refuses, before it opens a file or a device
    raw = tmp_path / "in.raw"
    np.zeros(8 * 8 * 8 * 3, np.uint8).tofile(raw)
    argv = [pkg.CLI_PATH, "encode", str(raw), str(tmp_path / "o.bin"), "8", "8", "8"]
    for extra, said in (({"DCT3D_CODEC_QUANT": "q=3"}, "exclude each other"),
                        ({"DCT3D_CODEC_RATE": "rate=1.5"}, "exclude each other"),
                        ({"DCT3D_CODEC_PSNR": "psnr=38"}, "exclude each other"),
                        ({"DCT3D_CODEC_SSIM": "ssim=abc"}, "Invalid ssim target 'ssim=abc': ssim=<target>, a decimal in (0, 1]"),
                        ({"DCT3D_CODEC_SSIM": "ssim=1.5"}, "Invalid ssim target 'ssim=1.5': ssim=<target>, a decimal in (0, 1]")):
        env = dict(os.environ, DCT3D_CODEC_SSIM="ssim=0.9")
        env.update(extra)
        r = subprocess.run(argv, env=env, capture_output=True, text=True)
        assert r.returncode == 1 and said in r.stdout and not (tmp_path / "o.bin").exists(), r.stdout
    argv = [pkg.CLI_PATH, "encode_rgb", str(raw), str(tmp_path / "o.bin"), "8", "8", "8"]
    for extra in ({"DCT3D_CODEC_PSNR_RGB": "psnr_rgb=38"}, {"DCT3D_CODEC_YCC": "1"},
                  {"DCT3D_CODEC_YCC": "1", "DCT3D_CODEC_CHROMA": "420"}):
        r = subprocess.run(argv, env=dict(os.environ, DCT3D_CODEC_SSIM="ssim=0.9", **extra), capture_output=True, text=True)
        assert r.returncode == 1 and "exclude each other" in r.stdout, r.stdout
        assert not (tmp_path / "o.bin.red").exists()


@pytest.mark.parametrize("args,said", [
    (["decode", "IN", "OUT", "8", "8", "8", "1", "8", "ssim=0.9"], "ssim= applies to encode"),
    (["decode_rgb", "IN", "OUT", "8", "8", "8", "1", "8", "ssim=0.9"], "ssim= applies to encode"),
    (["encode", "IN", "OUT", "8", "8", "8", "1,1", "8", "ssim=0.9"], "ssim= applies to encode"),
    (["decode", "IN", "OUT", "8", "8", "8", "1,1", "8", "ssim=0.9"], "ssim= applies to encode"),
    (["encode", "IN", "OUT", "8", "8", "8", "1", "8", "q=3", "ssim=0.9"], "q= and ssim= exclude each other"),
    (["encode", "IN", "OUT", "8", "8", "8", "1", "8", "ssim=0.9", "q=3"], "q= and ssim= exclude each other"),
    (["encode", "IN", "OUT", "8", "8", "8", "1", "8", "rate=1.5", "ssim=0.9"], "rate= and ssim= exclude each other"),
    (["encode_rgb", "IN", "OUT", "8", "8", "8", "1", "4", "ssim=0.9", "rate=1.5"], "rate= and ssim= exclude each other"),
    (["encode", "IN", "OUT", "8", "8", "8", "1", "8", "psnr=38", "ssim=0.9"], "psnr= and ssim= exclude each other"),
    (["encode_rgb", "IN", "OUT", "8", "8", "8", "1", "8", "ssim=0.9", "psnr_rgb=38"], "psnr_rgb= and ssim= exclude each other"),
    (["encode_rgb", "IN", "OUT", "8", "8", "8", "1", "8", "ycc=1", "ssim=0.9"], "ycc=1 and ssim= exclude each other"),
    (["encode_rgb", "IN", "OUT", "8", "8", "8", "1", "8", "ssim=0.9", "ycc=1", "chroma=420"], "ycc=1 and ssim= exclude each other"),
    (["encode_rgb", "IN", "OUT", "8", "8", "8", "1", "8", "ssim=0.9", "chroma=420"], "chroma=420 and ssim= exclude each other"),
    (["encode_rgb", "IN", "OUT", "8", "8", "8", "1", "4", "ssim="], "Invalid ssim target"),
    (["encode", "IN", "OUT", "8", "8", "8", "1", "8", "ssim=-1"], "Invalid ssim target"),
    (["encode", "IN", "OUT", "8", "8", "8", "1", "8", "ssim=0"], "Invalid ssim target"),
    (["encode", "IN", "OUT", "8", "8", "8", "1", "8", "ssim=1.01"], "Invalid ssim target"),
    (["encode", "IN", "OUT", "8", "8", "8", "1", "8", "ssim=abc"], "Invalid ssim target"),
])
def test_cli_rejects(pkg, tmp_path, args, said):
    """ssim= on a decode, with several devices, together with q=, rate=, psnr= or psnr_rgb=, with ycc=1 or chroma=420,
    or malformed: refused before any file is made"""
    raw = tmp_path / "in.raw"
    np.zeros(8 * 8 * 8 * 3, np.uint8).tofile(raw)
    out = tmp_path / "out.bin"
    argv = [str(raw) if a == "IN" else str(out) if a == "OUT" else a for a in args]
    r = subprocess.run([pkg.CLI_PATH] + argv, capture_output=True, text=True)
    assert r.returncode == 1 and said in r.stdout, r.stdout
    assert not out.exists() and not (tmp_path / "out.bin.red").exists()


def test_decode_entry_points_reject_an_ssim_target(pkg, tmp_path):
    """the library's decode and multi-device entry points refuse an SSIM target given by the environment"""
    raw = tmp_path / "in.bin"
    np.zeros(64, np.uint8).tofile(raw)
    env = dict(os.environ, DCT3D_CODEC_SSIM="ssim=0.9")
    for argv in (["decode", str(raw), str(tmp_path / "o.raw"), "8", "8", "8"],
                 ["decode", str(raw), str(tmp_path / "o.raw"), "8", "8", "8", "1,1"],
                 ["encode", str(raw), str(tmp_path / "o.raw"), "8", "8", "8", "1,1"]):
        r = subprocess.run([pkg.CLI_PATH] + argv, env=env, capture_output=True, text=True)
        assert r.returncode == 1 and "ssim= applies to single-device encodes only" in r.stdout, r.stdout
        assert not (tmp_path / "o.raw").exists()
