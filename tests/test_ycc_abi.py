"""CPU: the YCbCr colour option (DCT3D_OPT_COLOUR) is declared in the header and the package, the
option's argument checks that run without a device, codec_set_colour, and the CLI's rejections of ycc= where it has
no colour stage.  Nothing here needs a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_header_and_package_constants(pkg):
    header = open(os.path.join(pkg.INCLUDE_DIR, "dct3d.h")).read()
    opts = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define (DCT3D_OPT_\w+) (\d+)", header, re.M)}
    assert opts["DCT3D_OPT_COLOUR"] == 12 == pkg.DCT3D_OPT_COLOUR
    assert opts["DCT3D_OPT_COLOUR"] == max(v for k, v in opts.items() if k != "DCT3D_OPT_COLOUR") + 1  # the next id
    assert len(set(opts.values())) == len(opts)
    assert re.search(r"^#define DCT3D_COLOUR_PLANES 0$", header, re.M) and pkg.DCT3D_COLOUR_PLANES == 0
    assert re.search(r"^#define DCT3D_COLOUR_YCBCR 1$", header, re.M) and pkg.DCT3D_COLOUR_YCBCR == 1
    assert re.search(r"^#define DCT3D_ABI_VERSION 9$", header, re.M)  # additive
    for coef in ("19595 R + 38470 G +  7471 B", "-11059 R - 21709 G + 32768 B", "32768 R - 27439 G -  5329 B",
                 "91881 v", "-22554 u - 46802 v", "116130 u"):
        assert coef in header, coef  # the definition is in the header's block comment
    for name in ("rgb_to_ycbcr", "ycbcr_to_rgb"):
        assert callable(getattr(pkg, name))
    codec_h = open(os.path.join(pkg.INCLUDE_DIR, "codec.h")).read()
    assert re.search(r"^int codec_set_colour\(const char \*text\);", codec_h, re.M)
    assert "codec_set_colour" in _exported(pkg.CODEC_LIB_PATH)


def test_null_context_is_einval(pkg):
    L = pkg.lib()
    L.dct3d_ctx_set_option.argtypes = [C.c_void_p, C.c_int, C.c_double]
    assert L.dct3d_ctx_set_option(None, pkg.DCT3D_OPT_COLOUR, 1.0) == pkg.DCT3D_EINVAL


def test_option_values_with_a_device(pkg):
    """0 and 1 are taken, every other value is DCT3D_EINVAL and changes nothing (checked where a context can be made;
    tests/test_gpu_ycc.py checks the same on the GPU machine)"""
    L = pkg.lib()
    L.dct3d_ctx_set_option.argtypes = [C.c_void_p, C.c_int, C.c_double]
    h = C.c_void_p()
    if L.dct3d_ctx_create(0, 8, 8, 8, C.byref(h)) != pkg.DCT3D_OK:
        return
    try:
        for v in (1.0, 0.0, 1.0):
            assert L.dct3d_ctx_set_option(h, pkg.DCT3D_OPT_COLOUR, v) == pkg.DCT3D_OK
        for v in (2.0, 0.5, -1.0, 255.0, float("nan")):
            assert L.dct3d_ctx_set_option(h, pkg.DCT3D_OPT_COLOUR, v) == pkg.DCT3D_EINVAL, v
    finally:
        L.dct3d_ctx_destroy(h)


def test_codec_set_colour(pkg):
    pkg.lib()
    L = C.CDLL(pkg.CODEC_LIB_PATH)
    L.codec_set_colour.argtypes = [C.c_char_p]
    try:
        for text in (b"ycc=1", b"ycc=0", b"", None):
            assert L.codec_set_colour(text) == 0
        assert L.codec_set_colour(b"ycc=" + b"1" * 64) == 1  # too long: nothing changes
    finally:
        L.codec_set_colour(None)


@pytest.mark.parametrize("args,env,said", [
    (["encode_rgb", "IN", "OUT", "8", "8", "16", "1", "8", "psnr=30", "ycc=1"], {}, "ycc=1 and psnr= exclude each other"),
    (["encode_rgb", "IN", "OUT", "8", "8", "16", "1", "8", "ycc=1", "psnr=30"], {}, "ycc=1 and psnr= exclude each other"),
    (["encode_rgb", "IN", "OUT", "8", "8", "16", "1", "8", "psnr=30", "qmap=MAP", "ycc=1"], {}, "ycc=1 and psnr= exclude each other"),
    (["encode", "IN", "OUT", "8", "8", "16", "1", "8", "ycc=1"], {}, "ycc= applies to encode_rgb and decode_rgb on one device"),
    (["decode", "IN", "OUT", "8", "8", "16", "1", "8", "q=3", "ycc=1"], {}, "ycc= applies to encode_rgb and decode_rgb on one device"),
    (["encode", "IN", "OUT", "8", "8", "16", "1,1", "8", "ycc=1"], {}, "ycc= applies to encode_rgb and decode_rgb on one device"),
    (["encode_rgb", "IN", "OUT", "8", "8", "16", "1,1", "8", "ycc=1"], {}, "ycc= applies to encode_rgb and decode_rgb on one device"),
    (["decode_rgb", "IN", "OUT", "8", "8", "16", "1,1", "8", "ycc=1"], {}, "ycc= applies to encode_rgb and decode_rgb on one device"),
    (["encode_rgb", "IN", "OUT", "8", "8", "16", "1", "8", "ycc=2"], {}, "Invalid colour mode 'ycc=2'"),
    (["encode_rgb", "IN", "OUT", "8", "8", "16", "1", "8", "ycc="], {}, "Invalid colour mode 'ycc='"),
    (["decode_rgb", "IN", "OUT", "8", "8", "16", "1", "8", "ycc=yes"], {}, "Invalid colour mode 'ycc=yes'"),
    (["encode", "IN", "OUT", "8", "8", "16", "1", "8"], {"DCT3D_CODEC_YCC": "1"}, "ycc= applies to encode_rgb and decode_rgb on one device"),
    (["decode", "IN", "OUT", "8", "8", "16", "1", "8"], {"DCT3D_CODEC_YCC": "ycc=1"}, "ycc= applies to encode_rgb and decode_rgb on one device"),
    (["encode", "IN", "OUT", "8", "8", "16", "1,1", "8"], {"DCT3D_CODEC_YCC": "1"}, "ycc= applies to encode_rgb and decode_rgb on one device"),
    (["decode", "IN", "OUT", "8", "8", "16", "1,1", "8"], {"DCT3D_CODEC_YCC": "1"}, "ycc= applies to encode_rgb and decode_rgb on one device"),
    (["encode_rgb", "IN", "OUT", "8", "8", "16", "1", "8"], {"DCT3D_CODEC_YCC": "2"}, "Invalid colour mode '2'"),
    (["encode_rgb", "IN", "OUT", "8", "8", "16", "1", "8", "psnr=30"], {"DCT3D_CODEC_YCC": "1"}, "ycc=1 and psnr= exclude each other"),
    (["encode_rgb", "IN", "OUT", "8", "8", "16", "1", "8", "ycc=1"], {"DCT3D_CODEC_HOST_EG": "1"}, "DCT3D_CODEC_HOST_EG"),
    (["decode_rgb", "IN", "OUT", "8", "8", "16", "1", "8", "ycc=1"], {"DCT3D_CODEC_HOST_EG": "1"}, "DCT3D_CODEC_HOST_EG"),
])
def test_cli_rejects(pkg, tmp_path, args, env, said):
    """ycc=1 with psnr=, on a grey command, with several devices, on the host Exp-Golomb path, or a malformed value:
    a line of the kind the other tokens print, status 1, before any output file is made (and before a device is
    needed)"""
    raw, out, good = tmp_path / "in.raw", tmp_path / "out.bin", tmp_path / "map.txt"
    np.zeros(8 * 8 * 16 * 3, np.uint8).tofile(raw)
    good.write_text("5\n12\n")
    names = {"IN": str(raw), "OUT": str(out), "qmap=MAP": "qmap=" + str(good)}
    argv = [names.get(a, a) for a in args]
    clean = {k: v for k, v in os.environ.items() if not k.startswith("DCT3D_CODEC_")}
    r = subprocess.run([pkg.CLI_PATH] + argv, capture_output=True, text=True, env=dict(clean, **env))
    assert r.returncode == 1 and said in r.stdout, r.stdout
    assert not out.exists() and not any((tmp_path / ("out.bin" + s)).exists() for s in (".red", ".green", ".blue"))


def test_usage_names_the_token(pkg):
    r = subprocess.run([pkg.CLI_PATH], capture_output=True, text=True)
    assert r.returncode == 0 and "ycc=1" in r.stdout
