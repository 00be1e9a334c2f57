"""CPU: the fused stream entry points for frames of any size and packed RGB24 (dct3d_encode_eg_frames* /
dct3d_decode_eg_frames* / dct3d_eg_fetch_channel) are exported, declared in include/dct3d.h, listed in
ABI_SYMBOLS, and validate their arguments without a device."""
import ctypes as C
import os
import re
import subprocess

EG_FRAME_SYMBOLS = ("dct3d_encode_eg_frames_dev", "dct3d_encode_eg_frames", "dct3d_eg_fetch_channel",
                    "dct3d_decode_eg_frames_dev", "dct3d_decode_eg_frames")


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_eg_frame_symbols_exported_declared_and_listed(pkg):
    assert set(EG_FRAME_SYMBOLS) <= _exported(pkg.LIB_PATH)
    assert set(EG_FRAME_SYMBOLS) <= set(pkg.ABI_SYMBOLS)
    header = open(os.path.join(pkg.INCLUDE_DIR, "dct3d.h")).read()
    for name in EG_FRAME_SYMBOLS:
        assert re.search(r"^int %s\(dct3d_ctx \*ctx," % name, header, re.M), name


class _Args:
    """valid arguments of every call for `channels` channels of 13 x 11 frames, one 8-deep stack"""

    def __init__(self, channels=3):
        self.buf = (C.c_uint8 * (16 * 16 * 8 * 3 * 4))()
        self.p = C.cast(self.buf, C.c_void_p)
        self.cb = (C.c_uint8 * 3)(0, 0xA0, 0xFE)
        self.cn = (C.c_int * 3)(0, 3, 7)
        self.outs = (C.c_void_p * 3)(self.p.value, self.p.value + 4096, self.p.value + 8192)
        self.caps = (C.c_uint64 * 3)(4096, 4096, 4096)
        self.tb = (C.c_uint64 * 3)()
        self.nb = (C.c_uint64 * 3)(4096, 4096, 4096)
        self.sb64 = (C.c_uint64 * 3)(0, 3, 7)
        self.sb = (C.c_int * 3)(0, 3, 7)
        self.w, self.h, self.ch, self.n = 13, 11, channels, 1

    def calls(self, L, h):
        """name -> (function, argument list); index of width, height, channels, the frames and each array"""
        a = self
        return {
            "dct3d_encode_eg_frames_dev": [L.dct3d_encode_eg_frames_dev, [h, a.p, a.w, a.h, a.ch, a.n, a.cb, a.cn, a.outs, a.caps, a.tb],
                                           dict(w=2, h=3, ch=4, frames=1, arrays=(6, 7, 8, 9, 10))],
            "dct3d_encode_eg_frames": [L.dct3d_encode_eg_frames, [h, a.p, a.w, a.h, a.ch, a.n, a.cb, a.cn, a.tb],
                                       dict(w=2, h=3, ch=4, frames=1, arrays=(6, 7, 8))],
            "dct3d_decode_eg_frames_dev": [L.dct3d_decode_eg_frames_dev, [h, a.outs, a.nb, a.sb64, a.w, a.h, a.ch, a.n, a.p, a.tb],
                                           dict(w=4, h=5, ch=6, frames=8, arrays=(1, 2, 3, 9))],
            "dct3d_decode_eg_frames": [L.dct3d_decode_eg_frames, [h, a.outs, a.nb, a.sb, a.w, a.h, a.ch, a.n, a.p, a.tb],
                                       dict(w=4, h=5, ch=6, frames=8, arrays=(1, 2, 3, 9))],
        }


def _with(args, i, v):
    b = list(args)
    b[i] = v
    return b


def test_null_context_is_einval(pkg):
    L = pkg.lib()
    for channels in (1, 3):
        a = _Args(channels)
        for name, (f, args, ix) in a.calls(L, None).items():
            assert f(*args) == pkg.DCT3D_EINVAL, name
            assert f(*[None if i in ix["arrays"] or i == ix["frames"] else v for i, v in enumerate(args)]) == pkg.DCT3D_EINVAL, name
    assert L.dct3d_eg_fetch_channel(None, 0, None, 0) == pkg.DCT3D_EINVAL
    assert L.dct3d_eg_fetch_channel(None, 1, _Args().p, 4) == pkg.DCT3D_EINVAL


def test_bad_arguments_with_a_device(pkg):
    L = pkg.lib()
    h = C.c_void_p()
    if L.dct3d_ctx_create(0, 8, 8, 8, C.byref(h)) != pkg.DCT3D_OK:  # (no device here: the NULL-context test stands)
        return
    try:
        for channels in (1, 3):
            a = _Args(channels)
            for name, (f, args, ix) in a.calls(L, h).items():
                E = pkg.DCT3D_EINVAL
                assert f(*_with(args, ix["ch"], 2)) == E, name
                assert f(*_with(args, ix["ch"], 0)) == E, name
                assert f(*_with(args, ix["w"], 0)) == E, name
                assert f(*_with(args, ix["h"], 0)) == E, name
                assert f(*_with(args, ix["w"], -5)) == E, name
                assert f(*_with(args, ix["frames"], None)) == E, name
                for i in ix["arrays"]:  # a NULL array
                    assert f(*_with(args, i, None)) == E, (name, i)
                # channels x padded cubes past the cube-index limit
                big = _with(_with(_with(args, ix["w"], 8 * 1024 - 3), ix["h"], 8 * 1024 - 1), ix["ch"], 3)
                big[ix["ch"] + 1] = 100
                assert f(*big) == E, name
            # carry_bits 8, a misaligned stream pointer
            for name in ("dct3d_encode_eg_frames_dev", "dct3d_encode_eg_frames"):
                f, args, ix = a.calls(L, h)[name]
                bad = (C.c_int * 3)(0, 3, 7)
                bad[channels - 1] = 8
                assert f(*_with(args, 7, bad)) == pkg.DCT3D_EINVAL, name
                bad[channels - 1] = -1
                assert f(*_with(args, 7, bad)) == pkg.DCT3D_EINVAL, name
            odd = (C.c_void_p * 3)(a.p.value, a.p.value + 4096, a.p.value + 8192)
            odd[channels - 1] += 2
            f, args, ix = a.calls(L, h)["dct3d_encode_eg_frames_dev"]
            assert f(*_with(args, 8, odd)) == pkg.DCT3D_EINVAL
            f, args, ix = a.calls(L, h)["dct3d_decode_eg_frames_dev"]
            assert f(*_with(args, 1, odd)) == pkg.DCT3D_EINVAL
            f, args, ix = a.calls(L, h)["dct3d_decode_eg_frames"]
            bad = (C.c_int * 3)(0, 3, 7)
            bad[channels - 1] = 8
            assert f(*_with(args, 3, bad)) == pkg.DCT3D_EINVAL
        assert L.dct3d_eg_fetch_channel(h, 3, None, 0) == pkg.DCT3D_EINVAL
        assert L.dct3d_eg_fetch_channel(h, -1, None, 0) == pkg.DCT3D_EINVAL
        assert L.dct3d_eg_fetch_channel(h, 1, _Args().p, 1) == pkg.DCT3D_EINVAL  # nothing encoded yet
        assert L.dct3d_eg_fetch_channel(h, 2, None, 0) == pkg.DCT3D_OK
    finally:
        L.dct3d_ctx_destroy(h)
