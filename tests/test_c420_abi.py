"""CPU: 4:2:0 chroma subsampling (dct3d_ctx_set_chroma) is declared in the header and the package and
exported by the library; the argument checks that run without a device; codec_set_chroma; and the CLI's rejections of
chroma= where it cannot apply.  Nothing here needs a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

NEW = ("dct3d_ctx_set_chroma", "dct3d_ctx_get_chroma", "dct3d_chroma_size")


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_header_and_package_constants(pkg):
    header = open(os.path.join(pkg.INCLUDE_DIR, "dct3d.h")).read()
    assert re.search(r"^#define DCT3D_CHROMA_444 0$", header, re.M) and pkg.DCT3D_CHROMA_444 == 0
    assert re.search(r"^#define DCT3D_CHROMA_420 1$", header, re.M) and pkg.DCT3D_CHROMA_420 == 1
    assert re.search(r"^#define DCT3D_ABI_VERSION 9$", header, re.M)  # additive
    # a mode of the context, not an option id: DCT3D_OPT_COLOUR is still the highest
    opts = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define (DCT3D_OPT_\w+) (\d+)", header, re.M)}
    assert max(opts.values()) == opts["DCT3D_OPT_COLOUR"] == 12 and len(opts) == 9
    for decl in (r"^int dct3d_ctx_set_chroma\(dct3d_ctx \*ctx, int mode\);", r"^int dct3d_ctx_get_chroma\(const dct3d_ctx \*ctx, int \*mode\);",
                 r"^int dct3d_chroma_size\(int w, int h, int \*cw, int \*ch\);"):
        assert re.search(decl, header, re.M), decl
    for text in ("cw = (width + 1) / 2, ch = (height + 1) / 2", "p[2j][2i] + p[2j][2i+1] + p[2j+1][2i] + p[2j+1][2i+1] + 2) >> 2",
                 "p[y][x] = c[y >> 1][x >> 1]"):
        assert text in header, text  # the definition is in the header's block comment
    for name in ("chroma_size", "subsample_420", "upsample_420", "rgb_to_ycbcr420", "ycbcr420_to_rgb"):
        assert callable(getattr(pkg, name))
    assert callable(pkg.Context.set_chroma) and callable(pkg.Context.chroma)


def test_symbols_exported_and_listed(pkg):
    exp = _exported(pkg.LIB_PATH)
    for name in NEW:
        assert name in exp and name in pkg.ABI_SYMBOLS, name
    assert pkg.lib().dct3d_abi_version() == 9
    codec_h = open(os.path.join(pkg.INCLUDE_DIR, "codec.h")).read()
    assert re.search(r"^int codec_set_chroma\(const char \*text\);", codec_h, re.M)
    assert "codec_set_chroma" in _exported(pkg.CODEC_LIB_PATH)


def test_refusals_without_a_device(pkg):
    L = pkg.lib()
    E = pkg.DCT3D_EINVAL
    m, cw, ch = C.c_int(-7), C.c_int(0), C.c_int(0)
    assert L.dct3d_ctx_set_chroma(None, pkg.DCT3D_CHROMA_420) == E
    assert L.dct3d_ctx_set_chroma(None, 7) == E
    assert L.dct3d_ctx_get_chroma(None, C.byref(m)) == E and m.value == -7
    for w, h, want in ((1, 1, (1, 1)), (2, 2, (1, 1)), (15, 9, (8, 5)), (16, 16, (8, 8)), (17, 16, (9, 8)), (1366, 24, (683, 12)),
                       (2 ** 31 - 1, 1, (2 ** 30, 1))):
        assert L.dct3d_chroma_size(w, h, C.byref(cw), C.byref(ch)) == pkg.DCT3D_OK and (cw.value, ch.value) == want
        assert pkg.chroma_size(w, h) == want
    for w, h in ((0, 1), (1, 0), (-2, 4)):
        assert L.dct3d_chroma_size(w, h, C.byref(cw), C.byref(ch)) == E
    assert L.dct3d_chroma_size(4, 4, None, C.byref(ch)) == E and L.dct3d_chroma_size(4, 4, C.byref(cw), None) == E


def test_mode_values_with_a_device(pkg):
    """0 and 1 are taken, every other value is DCT3D_EINVAL and changes nothing (checked where a context can be made;
    tests/test_gpu_c420.py checks the same on the GPU machine)"""
    L = pkg.lib()
    h = C.c_void_p()
    if L.dct3d_ctx_create(0, 8, 8, 8, C.byref(h)) != pkg.DCT3D_OK:
        return
    try:
        m = C.c_int(-1)
        assert L.dct3d_ctx_get_chroma(h, C.byref(m)) == pkg.DCT3D_OK and m.value == pkg.DCT3D_CHROMA_444
        assert L.dct3d_ctx_set_chroma(h, pkg.DCT3D_CHROMA_420) == pkg.DCT3D_OK
        for v in (2, -1, 420):
            assert L.dct3d_ctx_set_chroma(h, v) == pkg.DCT3D_EINVAL
            assert L.dct3d_ctx_get_chroma(h, C.byref(m)) == pkg.DCT3D_OK and m.value == pkg.DCT3D_CHROMA_420
        assert L.dct3d_ctx_get_chroma(h, None) == pkg.DCT3D_EINVAL
    finally:
        L.dct3d_ctx_destroy(h)


def test_codec_set_chroma(pkg):
    pkg.lib()
    L = C.CDLL(pkg.CODEC_LIB_PATH)
    L.codec_set_chroma.argtypes = [C.c_char_p]
    try:
        for text in (b"chroma=420", b"chroma=444", b"", None):
            assert L.codec_set_chroma(text) == 0
        assert L.codec_set_chroma(b"chroma=" + b"4" * 64) == 1  # too long: nothing changes
    finally:
        L.codec_set_chroma(None)


RGB = ["IN", "OUT", "8", "8", "16", "1", "8"]
APPLIES = "chroma= applies to encode_rgb and decode_rgb on one device"
NEEDS = "chroma=420 needs ycc=1"


@pytest.mark.parametrize("args,env,said", [
    (["encode_rgb"] + RGB + ["ycc=1", "chroma=422"], {}, "Invalid chroma mode 'chroma=422'"),
    (["encode_rgb"] + RGB + ["ycc=1", "chroma="], {}, "Invalid chroma mode 'chroma='"),
    (["decode_rgb"] + RGB + ["ycc=1", "chroma=4:2:0"], {}, "Invalid chroma mode 'chroma=4:2:0'"),
    (["encode_rgb"] + RGB + ["ycc=1"], {"DCT3D_CODEC_CHROMA": "411"}, "Invalid chroma mode '411'"),
    (["encode_rgb"] + RGB + ["chroma=420"], {}, NEEDS),
    (["decode_rgb"] + RGB + ["chroma=420"], {}, NEEDS),
    (["encode_rgb"] + RGB + ["ycc=0", "chroma=420"], {}, NEEDS),
    (["encode_rgb"] + RGB + ["q=3", "chroma=420"], {}, NEEDS),
    (["encode_rgb"] + RGB, {"DCT3D_CODEC_CHROMA": "420"}, NEEDS),
    (["decode_rgb"] + RGB, {"DCT3D_CODEC_CHROMA": "chroma=420"}, NEEDS),
    (["encode"] + RGB + ["chroma=420"], {}, APPLIES),
    (["decode"] + RGB + ["q=3", "chroma=420"], {}, APPLIES),
    (["encode"] + RGB, {"DCT3D_CODEC_CHROMA": "420"}, APPLIES),
    (["decode"] + RGB, {"DCT3D_CODEC_CHROMA": "420"}, APPLIES),
    (["encode"] + RGB[:5] + ["1,1", "8", "chroma=420"], {}, APPLIES),
    (["encode_rgb"] + RGB[:5] + ["1,1", "8", "ycc=1", "chroma=420"], {}, "applies to encode_rgb and decode_rgb on one device"),
    (["decode_rgb"] + RGB[:5] + ["1,1", "8", "chroma=420"], {}, APPLIES),
    (["encode"] + RGB[:5] + ["1,1", "8"], {"DCT3D_CODEC_CHROMA": "420"}, APPLIES),
    (["decode"] + RGB[:5] + ["1,1", "8"], {"DCT3D_CODEC_CHROMA": "420"}, APPLIES),
    (["encode_rgb"] + RGB + ["ycc=1", "chroma=420"], {"DCT3D_CODEC_HOST_EG": "1"}, "DCT3D_CODEC_HOST_EG"),
    (["decode_rgb"] + RGB + ["ycc=1", "chroma=420"], {"DCT3D_CODEC_HOST_EG": "1"}, "DCT3D_CODEC_HOST_EG"),
    (["encode_rgb"] + RGB, {"DCT3D_CODEC_HOST_EG": "1", "DCT3D_CODEC_CHROMA": "420"}, "DCT3D_CODEC_HOST_EG"),
])
def test_cli_rejects(pkg, tmp_path, args, env, said):
    """a malformed value, chroma=420 without ycc=1, on a grey command, with several devices or on the host Exp-Golomb
    path: a line of the kind the other tokens print, status 1, before any output file is made (and before a device is
    needed)"""
    raw, out = tmp_path / "in.raw", tmp_path / "out.bin"
    np.zeros(8 * 8 * 16 * 3, np.uint8).tofile(raw)
    names = {"IN": str(raw), "OUT": str(out)}
    argv = [names.get(a, a) for a in args]
    clean = {k: v for k, v in os.environ.items() if not k.startswith("DCT3D_CODEC_")}
    r = subprocess.run([pkg.CLI_PATH] + argv, capture_output=True, text=True, env=dict(clean, **env))
    assert r.returncode == 1 and said in r.stdout, r.stdout
    assert not out.exists() and not any((tmp_path / ("out.bin" + s)).exists() for s in (".red", ".green", ".blue"))


def test_chroma_444_is_accepted_where_420_is_not(pkg, tmp_path):
    """chroma=444 is the default spelled out: a grey command takes it (and then fails later, for want of a device or
    not at all -- but never with a chroma message)"""
    raw, out = tmp_path / "in.raw", tmp_path / "out.bin"
    np.zeros(8 * 8 * 16, np.uint8).tofile(raw)
    clean = {k: v for k, v in os.environ.items() if not k.startswith("DCT3D_CODEC_")}
    r = subprocess.run([pkg.CLI_PATH, "encode", str(raw), str(out), "8", "8", "16", "1", "8", "chroma=444"],
                       capture_output=True, text=True, env=clean)
    assert "chroma" not in r.stdout, r.stdout


def test_usage_names_the_token(pkg):
    r = subprocess.run([pkg.CLI_PATH], capture_output=True, text=True)
    assert r.returncode == 0 and "chroma=420" in r.stdout and "ycc=1" in r.stdout
