"""CPU: the packed RGB24 entry points (ABI 9) are exported, validate their arguments without a device, and
the codec CLI knows encode_rgb / decode_rgb."""
import ctypes as C
import subprocess

RGB_SYMBOLS = ("dct3d_encode_stacks_rgb", "dct3d_encode_stacks_rgb_dev", "dct3d_decode_stacks_rgb",
               "dct3d_decode_stacks_rgb_dev")


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_rgb_symbols_exported(pkg):
    assert set(RGB_SYMBOLS) <= _exported(pkg.LIB_PATH)
    assert set(RGB_SYMBOLS) <= set(pkg.ABI_SYMBOLS)
    assert {"encode_rgb_ex", "decode_rgb_ex"} <= _exported(pkg.CODEC_LIB_PATH)


def test_abi_version_is_9(pkg):
    assert pkg.lib().dct3d_abi_version() == 9


def test_rgb_argument_validation_without_device(pkg):
    L = pkg.lib()
    buf = (C.c_uint8 * (8 * 8 * 8 * 3 * 4))()
    p = C.cast(buf, C.c_void_p)
    for name in RGB_SYMBOLS:  # a NULL context, whatever the buffers
        assert getattr(L, name)(None, p, 8, 8, 1, p) == pkg.DCT3D_EINVAL, name
        assert getattr(L, name)(None, None, 8, 8, 1, None) == pkg.DCT3D_EINVAL, name
    h = C.c_void_p()
    if L.dct3d_ctx_create(0, 8, 8, 8, C.byref(h)) == pkg.DCT3D_OK:  # (a device is present: NULL buffers, bad sizes)
        try:
            for name in RGB_SYMBOLS:
                assert getattr(L, name)(h, None, 8, 8, 1, p) == pkg.DCT3D_EINVAL, name
                assert getattr(L, name)(h, p, 8, 8, 1, None) == pkg.DCT3D_EINVAL, name
                assert getattr(L, name)(h, p, 12, 8, 1, p) == pkg.DCT3D_EINVAL, name
                # 3 x cubes past the 32-bit cube-index limit of the int32 side (the grey limit holds for cubes)
                assert getattr(L, name)(h, p, 8 * 1024, 8 * 1024, 100, p) == pkg.DCT3D_EINVAL, name
        finally:
            L.dct3d_ctx_destroy(h)


def test_cli_usage_names_rgb_commands(pkg):
    r = subprocess.run([pkg.CLI_PATH], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "encode_rgb" in r.stdout and "decode_rgb" in r.stdout


def test_cli_encode_rgb_missing_file_exits_1(pkg, tmp_path):
    r = subprocess.run([pkg.CLI_PATH, "encode_rgb", str(tmp_path / "missing.rgb"), str(tmp_path / "out"), "64", "64", "8"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Cannot open input file" in r.stdout and "missing.rgb" in r.stdout
    r = subprocess.run([pkg.CLI_PATH, "decode_rgb", str(tmp_path / "missing"), str(tmp_path / "out.rgb"), "64", "64", "8"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Cannot open input file" in r.stdout and "missing.red" in r.stdout
