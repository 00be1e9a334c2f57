"""CPU: the entry points for frames of any size (dct3d_encode_frames* / dct3d_decode_frames*) are exported and
validate their arguments without a device; pad_frames / padded_size define the padded raster; the codec CLI
accepts a size that is no multiple of 8."""
import ctypes as C
import subprocess

import numpy as np

FRAME_SYMBOLS = ("dct3d_encode_frames", "dct3d_encode_frames_dev", "dct3d_decode_frames", "dct3d_decode_frames_dev")


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_frame_symbols_exported(pkg):
    assert set(FRAME_SYMBOLS) <= _exported(pkg.LIB_PATH)
    assert set(FRAME_SYMBOLS) <= set(pkg.ABI_SYMBOLS)


def test_frame_argument_validation_without_device(pkg):
    L = pkg.lib()
    buf = (C.c_uint8 * (16 * 16 * 8 * 3 * 4))()
    p = C.cast(buf, C.c_void_p)
    for name in FRAME_SYMBOLS:  # a NULL context, whatever the rest
        for ch in (1, 3):
            assert getattr(L, name)(None, p, 13, 11, ch, 1, p) == pkg.DCT3D_EINVAL, name
        assert getattr(L, name)(None, None, 13, 11, 1, 1, None) == pkg.DCT3D_EINVAL, name
    h = C.c_void_p()
    if L.dct3d_ctx_create(0, 8, 8, 8, C.byref(h)) == pkg.DCT3D_OK:  # (a device is present)
        try:
            for name in FRAME_SYMBOLS:
                f = getattr(L, name)
                assert f(h, p, 13, 11, 2, 1, p) == pkg.DCT3D_EINVAL, name
                assert f(h, p, 13, 11, 0, 1, p) == pkg.DCT3D_EINVAL, name
                assert f(h, p, 0, 11, 1, 1, p) == pkg.DCT3D_EINVAL, name
                assert f(h, p, 13, 0, 3, 1, p) == pkg.DCT3D_EINVAL, name
                assert f(h, p, -5, 11, 1, 1, p) == pkg.DCT3D_EINVAL, name
                assert f(h, None, 13, 11, 1, 1, p) == pkg.DCT3D_EINVAL, name
                assert f(h, p, 13, 11, 1, 1, None) == pkg.DCT3D_EINVAL, name
                # channels x padded cubes past the cube-index limit (the grey limit holds for the cubes alone)
                assert f(h, p, 8 * 1024 - 3, 8 * 1024 - 1, 3, 100, p) == pkg.DCT3D_EINVAL, name
        finally:
            L.dct3d_ctx_destroy(h)


def test_padded_size(pkg):
    assert pkg.padded_size(1366, 768) == (1368, 768)
    assert pkg.padded_size(1680, 1050) == (1680, 1056)
    assert pkg.padded_size(1, 1) == (8, 8)
    assert pkg.padded_size(64, 64) == (64, 64)


def test_pad_frames_is_edge_padding(pkg):
    rng = np.random.default_rng(3)
    for w, h in ((13, 11), (5, 3), (16, 12), (12, 16), (64, 64)):
        wp, hp = pkg.padded_size(w, h)
        grey = rng.integers(0, 256, size=(4, h, w), dtype=np.uint8)
        assert np.array_equal(pkg.pad_frames(grey), np.pad(grey, ((0, 0), (0, hp - h), (0, wp - w)), mode="edge"))
        rgb = rng.integers(0, 256, size=(4, h, w, 3), dtype=np.uint8)
        ref = np.pad(rgb, ((0, 0), (0, hp - h), (0, wp - w), (0, 0)), mode="edge")
        got = pkg.pad_frames(rgb)
        assert got.shape == (4, hp, wp, 3) and np.array_equal(got, ref)
        for ch in range(3):  # per channel: the channel axis is never padded
            assert np.array_equal(got[..., ch], pkg.pad_frames(np.ascontiguousarray(rgb[..., ch])))


def test_cli_accepts_a_size_that_is_no_multiple_of_8(pkg, tmp_path):
    """the geometry passes, the missing input file is what stops the command"""
    for cmd, missing in (("encode", "missing.raw"), ("decode", "missing.bin"), ("encode_rgb", "missing.rgb")):
        r = subprocess.run([pkg.CLI_PATH, cmd, str(tmp_path / missing), str(tmp_path / "out"), "13", "11", "8"],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "Cannot open input file" in r.stdout and missing in r.stdout, r.stdout
        assert "Invalid geometry" not in r.stdout
    r = subprocess.run([pkg.CLI_PATH, "decode_rgb", str(tmp_path / "missing"), str(tmp_path / "out.rgb"), "13", "11", "8"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Cannot open input file" in r.stdout and "missing.red" in r.stdout
    r = subprocess.run([pkg.CLI_PATH, "encode", str(tmp_path / "missing.raw"), str(tmp_path / "out"), "0", "11", "8"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Invalid geometry" in r.stdout
