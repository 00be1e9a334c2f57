"""CPU: the per-(stack, channel) quantiser calls (dct3d_*_eg_frames_vqc*) are exported, declared and listed
and validate their arguments (the one test that needs a context for that is marked gpu);
pick_stack_channel_qualities against a direct restatement of its rule; the codec's qmap3= parser and every refusal of
the CLI, matched by the new refusal lines' own words."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

VQC_SYMBOLS = ("dct3d_encode_eg_frames_vqc_dev", "dct3d_encode_eg_frames_vqc", "dct3d_decode_eg_frames_vqc_dev",
               "dct3d_decode_eg_frames_vqc")
LADDER = (1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 24, 32, 40, 48, 64)


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_vqc_symbols_exported_declared_and_listed(pkg):
    assert set(VQC_SYMBOLS) <= _exported(pkg.LIB_PATH)
    assert set(VQC_SYMBOLS) <= set(pkg.ABI_SYMBOLS)
    header = open(os.path.join(pkg.INCLUDE_DIR, "dct3d.h")).read()
    for name in VQC_SYMBOLS:
        m = re.search(r"^int %s\(dct3d_ctx \*ctx,[^;]*;" % name, header, re.M)
        assert m and "const uint8_t *table_map" in m.group(0) and "stack_table" not in m.group(0), name
    assert re.search(r"^#define DCT3D_ABI_VERSION 9$", header, re.M)  # additive: detected by symbol
    assert pkg.lib().dct3d_abi_version() == 9
    assert {"codec_parse_qmap3", "codec_set_qmap3"} <= _exported(pkg.CODEC_LIB_PATH)
    for name in ("encode_eg_frames_vqc", "encode_eg_frames_vqc_dev", "decode_eg_frames_vqc", "decode_eg_frames_vqc_dev"):
        assert callable(getattr(pkg.Context, name))
    assert callable(pkg.pick_stack_channel_qualities)


def _calls(pkg, h, n_tables=2, n_stacks=2):
    """the four calls on 13 x 11 RGB frames, each as (function, argument list, index of tables / n_tables / map)"""
    L = pkg.lib()
    vp = lambda a: C.cast(a, C.c_void_p)
    fr = (C.c_uint8 * (13 * 11 * 3 * 8 * n_stacks))()
    tabs = (C.c_int32 * (33 * 22))(*([7] * (33 * 22)))
    tmap = (C.c_uint8 * 24)(*([1] * 24))
    cb, cn = (C.c_uint8 * 3)(), (C.c_int * 3)()
    outs, caps, tb = (C.c_void_p * 3)(), (C.c_uint64 * 3)(), (C.c_uint64 * 3)()
    nb, sb64, sb32, eb = (C.c_uint64 * 3)(64, 64, 64), (C.c_uint64 * 3)(), (C.c_int * 3)(), (C.c_uint64 * 3)()
    streams = (C.c_void_p * 3)(*[C.cast((C.c_uint8 * 64)(), C.c_void_p).value] * 3)
    keep = (fr, tabs, tmap, cb, cn, outs, caps, tb, nb, sb64, sb32, eb, streams)
    head = [h, vp(fr), 13, 11, 3, n_stacks, vp(tabs), n_tables, vp(tmap)]
    dhead = [13, 11, 3, n_stacks, vp(tabs), n_tables, vp(tmap)]
    return [
        (L.dct3d_encode_eg_frames_vqc, head + [vp(cb), vp(cn), vp(tb)], (6, 7, 8)),
        (L.dct3d_encode_eg_frames_vqc_dev, head + [vp(cb), vp(cn), vp(outs), vp(caps), vp(tb)], (6, 7, 8)),
        (L.dct3d_decode_eg_frames_vqc, [h, vp(streams), vp(nb), vp(sb32)] + dhead + [vp(fr), vp(eb)], (8, 9, 10)),
        (L.dct3d_decode_eg_frames_vqc_dev, [h, vp(streams), vp(nb), vp(sb64)] + dhead + [vp(fr), vp(eb)], (8, 9, 10)),
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


@pytest.mark.gpu
def test_bad_arguments_with_a_device(pkg):
    """Every argument error that needs a context is DCT3D_EINVAL, through the C-ABI itself (the one test of this module
    that needs a device).  The map is [n_stacks][3]: its LAST entry, (stack 1, channel 2), is checked too."""
    L = pkg.lib()
    h = C.c_void_p()
    assert L.dct3d_ctx_create(0, 8, 8, 8, C.byref(h)) == pkg.DCT3D_OK
    try:
        E = pkg.DCT3D_EINVAL
        calls, keep = _calls(pkg, h)
        for f, args, (it, nt, im) in calls:
            for i, v in ((it, None), (im, None), (nt, 0), (nt, 33), (nt, -1), (nt, 1)):  # (n_tables = 1: the map's 1s)
                assert f(*_with(args, i, v)) == E, (f.__name__, i, v)
        for at in (0, 4, 5):
            calls, keep = _calls(pkg, h)
            keep[2][at] = 2  # an entry == n_tables
            for f, args, _ in calls:
                assert f(*args) == E, (f.__name__, at)
        assert L.dct3d_ctx_set_option(h, pkg.DCT3D_OPT_EG_TWO_STEP, 1.0) == pkg.DCT3D_OK
        calls, keep = _calls(pkg, h)
        for f, args, _ in calls:
            assert f(*args) == E, f.__name__  # the option is refused, not ignored
    finally:
        L.dct3d_ctx_destroy(h)


# ---- pick_stack_channel_qualities ---------------------------------------------------------------------------------

def _bumpy(rng, stacks):
    """[T, stacks, 3] sums that are not monotone in the quality"""
    a = rng.integers(0, 5000, size=(len(LADDER), stacks, 3)).astype(np.uint64)
    a[:, 0, :] = 0          # a stack every candidate fits
    a[:, 1, :] = 2**40      # a stack no candidate fits
    return a


def _restated(bits, qualities, target, rungs):
    """the rule as the interface states it, written out"""
    T, res = len(qualities), []
    for s in range(bits.shape[1]):
        best = None
        for i in range(T):
            j = min(i + rungs, T - 1)
            cost = int(bits[i, s, 0]) + int(bits[j, s, 1]) + int(bits[j, s, 2])
            if cost <= target and (best is None or qualities[i] < qualities[best]):
                best = i
        if best is None:
            best = max(range(T), key=lambda i: qualities[i])
        j = min(best + rungs, T - 1)
        res.append((qualities[best], qualities[j], qualities[j]))
    return res


def test_pick_stack_channel_qualities(pkg):
    rng = np.random.default_rng(20261022)
    bits = _bumpy(rng, 9)
    assert not all(np.all(np.diff(bits[:, s].sum(axis=1).astype(np.int64)) <= 0) for s in range(2, 9))
    shuffled = (5, 64, 1, 12, 3, 48, 2, 40, 4, 32, 6, 24, 8, 20, 10, 16)  # the order given, not the ladder's
    for quals in (LADDER, shuffled, LADDER[:5]):
        b = bits[:len(quals)]
        for rungs in (0, 1, 2, 7, 15, 40):
            for target in (0, 1, 2500.5, 7000, 9000, 2**41 * 3):
                got = pkg.pick_stack_channel_qualities(b, quals, target, rungs)
                assert got == _restated(b, list(quals), target, rungs), (quals, rungs, target)
                assert all(isinstance(q, int) for t in got for q in t)
                if rungs == 0:
                    assert [t[0] for t in got] == pkg.pick_stack_qualities(b, quals, target)
                    assert all(t[0] == t[1] == t[2] for t in got)
    assert pkg.pick_stack_channel_qualities(bits, LADDER, 7000) == pkg.pick_stack_channel_qualities(bits, LADDER, 7000, 0)
    # the clamp at the ladder's end: the stack nothing fits takes the last rung for all three, the stack everything
    # fits the first and the rung `chroma_rungs` on -- or the last
    got = pkg.pick_stack_channel_qualities(bits, LADDER, 2500, 2)
    assert got[0] == (1, 3, 3) and got[1] == (64, 64, 64)
    assert pkg.pick_stack_channel_qualities(bits, LADDER, 2500, 15)[0] == (1, 64, 64)
    assert pkg.pick_stack_channel_qualities(bits, LADDER, 2500, 99)[0] == (1, 64, 64)
    for bad in (np.zeros((3, 2, 3)), np.zeros((16, 2, 1)), np.zeros((16, 2)), np.zeros((16, 2, 4))):
        with pytest.raises(ValueError):
            pkg.pick_stack_channel_qualities(bad, LADDER, 5)
    with pytest.raises(ValueError):
        pkg.pick_stack_channel_qualities(bits, LADDER, 5, -1)


def test_context_methods_refuse_a_wrong_map_before_the_library(pkg):
    """a wrong shape or value is Dct3dError(DCT3D_EINVAL), raised by the wrapper: no context handle is needed"""
    ctx = object.__new__(pkg.Context)
    ctx.bw, ctx.bh, ctx.bd, ctx._h = 8, 8, 8, None
    fr = np.zeros((16, 11, 13, 3), np.uint8)
    pal = np.stack([pkg.quant_table(q, 8) for q in (5, 12)])
    for m in (np.zeros(2, np.uint8), np.zeros((2, 1), np.uint8), np.zeros((3, 3), np.uint8), np.zeros((3, 2), np.uint8),
              np.full((2, 3), 256), np.full((2, 3), -1), np.full((2, 3), 0.5), None):
        with pytest.raises(pkg.Dct3dError) as e:
            ctx.encode_eg_frames_vqc(fr, pal, m)
        assert e.value.code == pkg.DCT3D_EINVAL
        with pytest.raises(pkg.Dct3dError) as e:
            ctx.decode_eg_frames_vqc([b"\0" * 8] * 3, 13, 11, 2, pal, m)
        assert e.value.code == pkg.DCT3D_EINVAL


# ---- the codec's qmap3= -------------------------------------------------------------------------------------------

def _codec(pkg):
    pkg.lib()
    L = C.CDLL(pkg.CODEC_LIB_PATH)
    L.codec_parse_qmap3.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_int)]
    L.codec_set_qmap3.argtypes = [C.c_char_p]
    L.codec_set_qmap.argtypes = [C.c_char_p]
    L.codec_set_quant.argtypes = [C.c_char_p]
    return L


def test_codec_parse_qmap3(pkg, tmp_path):
    L = _codec(pkg)
    f = tmp_path / "m.txt"
    out = (C.c_int * 7)()

    def parse(text, n=2):
        f.write_text(text)
        for i in range(7):
            out[i] = -7
        return L.codec_parse_qmap3(str(f).encode(), n, out), list(out)

    assert parse("5 64 1\n12 12 3\n") == (0, [5, 64, 1, 12, 12, 3, -7])
    assert parse("5 64 1\n12 12 3") == (0, [5, 64, 1, 12, 12, 3, -7])      # no newline after the last line
    assert parse("5 64 1\r\n12 12 3\r\n") == (0, [5, 64, 1, 12, 12, 3, -7])
    assert parse("1 1 64\n", 1) == (0, [1, 1, 64] + [-7] * 4)
    for bad in ("5 64\n12 12 3\n", "5 64 1\n12 12\n",                     # two columns
                "5 64 1 2\n12 12 3\n", "5 64 1\n12 12 3 4\n",             # four columns
                "5 7 1\n12 12 3\n", "5 64 0\n12 12 3\n", "65 64 1\n12 12 3\n", "5 64 1\n12 255 3\n",  # off the ladder
                "5 64 1\n", "5 64 1\n12 12 3\n1 1 1\n",                   # a line too few, a line too many
                "5\t64\t1\n12 12 3\n", "5 64\t1\n12 12 3\n",              # tabs
                "", "\n", "5 64 1\n\n12 12 3\n", " 5 64 1\n12 12 3\n", "5 64 1 \n12 12 3\n", "5  64 1\n12 12 3\n",
                "5 +64 1\n12 12 3\n", "5 -64 1\n12 12 3\n", "5 64 1.0\n12 12 3\n", "5,64,1\n12,12,3\n", "5\n64\n"):
        assert parse(bad) == (1, [-7] * 7), repr(bad)
    assert L.codec_parse_qmap3(str(tmp_path / "missing.txt").encode(), 2, out) == 1
    f.write_text("5 64 1\n12 12 3\n")
    assert L.codec_parse_qmap3(None, 2, out) == 1 and L.codec_parse_qmap3(str(f).encode(), 0, out) == 1
    assert L.codec_parse_qmap3(str(f).encode(), 2, None) == 1


def test_codec_set_qmap3_and_cq_keep_a_text_or_say_too_long(pkg):
    """the setters keep the text; what the map excludes is refused by the call that finds both (test_cli_rejects)"""
    L = _codec(pkg)
    L.codec_set_cq.argtypes = [C.c_char_p]
    try:
        assert L.codec_set_qmap3(b"qmap3=/tmp/x") == 0
        assert L.codec_set_qmap3(b"qmap3=" + b"x" * 5000) == 1  # too long: nothing changes
        assert L.codec_set_cq(b"cq=2") == 0 and L.codec_set_cq(b"cq=" + b"1" * 40) == 1
    finally:
        L.codec_set_qmap3(None)
        L.codec_set_cq(None)


RGB = ["IN", "OUT", "8", "8", "16", "1", "8"]


@pytest.mark.parametrize("args,env,said", [
    # cq= without ycc=1
    (["encode_rgb"] + RGB + ["rate=2", "qmap3=MAP", "cq=2"], {}, "cq= needs ycc=1"),
    (["encode_rgb"] + RGB + ["ycc=0", "rate=2", "qmap3=MAP", "cq=2"], {}, "cq= needs ycc=1"),
    (["encode_rgb"] + RGB + ["rate=2", "qmap3=MAP"], {"DCT3D_CODEC_CQ": "cq=2"}, "cq= needs ycc=1"),
    # cq= without rate= + qmap3=
    (["encode_rgb"] + RGB + ["ycc=1", "qmap3=MAP", "cq=2"], {}, "cq= applies to"),
    (["encode_rgb"] + RGB + ["ycc=1", "rate=2", "cq=2"], {}, "cq= applies to"),
    (["encode_rgb"] + RGB + ["ycc=1", "rate=2", "qmap=MAP1", "cq=2"], {}, "cq= applies to"),
    (["decode_rgb"] + RGB + ["ycc=1", "qmap3=MAP", "cq=2"], {}, "cq= applies to"),
    (["encode_rgb"] + RGB + ["ycc=1", "qmap3=MAP"], {"DCT3D_CODEC_CQ": "2"}, "cq= applies to"),
    (["encode_rgb"] + RGB + ["ycc=1", "rate=2", "qmap3=MAP", "cq=16"], {}, "Invalid chroma offset"),
    (["encode_rgb"] + RGB + ["ycc=1", "rate=2", "qmap3=MAP", "cq=-1"], {}, "Invalid chroma offset"),
    (["encode_rgb"] + RGB + ["ycc=1", "rate=2", "qmap3=MAP", "cq=2x"], {}, "Invalid chroma offset"),
    # qmap3= together with qmap=, q= or psnr=
    (["encode_rgb"] + RGB + ["qmap3=MAP", "qmap=MAP1"], {}, "qmap3= excludes"),
    (["decode_rgb"] + RGB + ["qmap=MAP1", "qmap3=MAP"], {}, "qmap3= excludes"),
    (["encode_rgb"] + RGB + ["q=3", "qmap3=MAP"], {}, "qmap3= excludes"),
    (["decode_rgb"] + RGB + ["qmap3=MAP", "q=3"], {}, "qmap3= excludes"),
    (["encode_rgb"] + RGB + ["psnr=30", "qmap3=MAP"], {}, "qmap3= excludes"),
    (["encode_rgb"] + RGB, {"DCT3D_CODEC_QMAP3": "qmap3=MAP", "DCT3D_CODEC_QMAP": "qmap=MAP1"}, "qmap3= excludes"),
    (["encode_rgb"] + RGB, {"DCT3D_CODEC_QMAP3": "qmap3=MAP", "DCT3D_CODEC_QUANT": "q=3"}, "qmap3= excludes"),
    (["encode_rgb"] + RGB, {"DCT3D_CODEC_QMAP3": "qmap3=MAP", "DCT3D_CODEC_PSNR": "psnr=30"}, "qmap3= excludes"),
    # on a grey command
    (["encode"] + RGB + ["qmap3=MAP"], {}, "qmap3= and cq= apply to"),
    (["decode"] + RGB + ["qmap3=MAP"], {}, "qmap3= and cq= apply to"),
    (["encode"] + RGB, {"DCT3D_CODEC_QMAP3": "qmap3=MAP"}, "qmap3= and cq= apply to"),
    (["decode"] + RGB, {"DCT3D_CODEC_QMAP3": "qmap3=MAP"}, "qmap3= and cq= apply to"),
    # on a several-device command
    (["encode_rgb", "IN", "OUT", "8", "8", "16", "1,1", "8", "qmap3=MAP"], {}, "qmap3= and cq= apply to"),
    (["decode_rgb", "IN", "OUT", "8", "8", "16", "1,1", "8", "qmap3=MAP"], {}, "qmap3= and cq= apply to"),
    (["encode", "IN", "OUT", "8", "8", "16", "1,1", "8"], {"DCT3D_CODEC_QMAP3": "qmap3=MAP"}, "qmap3= and cq= apply to"),
    (["decode", "IN", "OUT", "8", "8", "16", "1,1", "8"], {"DCT3D_CODEC_QMAP3": "qmap3=MAP"}, "qmap3= and cq= apply to"),
    (["encode", "IN", "OUT", "8", "8", "16", "1,1", "8", "qmap3=MAP"], {}, "qmap3= and cq= apply to"),
    (["decode", "IN", "OUT", "8", "8", "16", "1,1", "8", "qmap3=MAP"], {}, "qmap3= and cq= apply to"),
    # on the host Exp-Golomb path
    (["encode_rgb"] + RGB + ["qmap3=MAP"], {"DCT3D_CODEC_HOST_EG": "1"}, "DCT3D_CODEC_HOST_EG"),
    (["decode_rgb"] + RGB + ["qmap3=MAP"], {"DCT3D_CODEC_HOST_EG": "1"}, "DCT3D_CODEC_HOST_EG"),
    # a malformed file
    (["encode_rgb"] + RGB + ["qmap3="], {}, "Invalid quality map"),
    (["encode_rgb", "IN", "OUT", "8", "8", "24", "1", "8", "qmap3=MAP"], {}, "Invalid quality map file"),  # 3 stacks, 2 lines
    (["decode_rgb", "IN", "OUT", "8", "8", "24", "1", "8", "qmap3=MAP"], {}, "Invalid quality map file"),
    (["decode_rgb"] + RGB + ["qmap3=BAD"], {}, "Invalid quality map file"),     # a 7
    (["encode_rgb"] + RGB + ["qmap3=MAP1"], {}, "Invalid quality map file"),    # one column
    (["encode_rgb"] + RGB + ["qmap3=MISSING"], {}, "Invalid quality map file"),
])
def test_cli_rejects(pkg, tmp_path, args, env, said):
    """every refusal of qmap3= and cq=: a line, status 1, before any output file is made (and before a device is
    needed); the map files are left as they were"""
    raw, out = tmp_path / "in.raw", tmp_path / "out.bin"
    good, one, bad = tmp_path / "map3.txt", tmp_path / "map1.txt", tmp_path / "bad.txt"
    np.zeros(8 * 8 * 24 * 3, np.uint8).tofile(raw)
    good.write_text("5 12 12\n12 16 16\n")
    one.write_text("5\n12\n")
    bad.write_text("5 12 12\n5 7 7\n")
    names = {"IN": str(raw), "OUT": str(out), "qmap3=MAP": "qmap3=" + str(good), "qmap=MAP1": "qmap=" + str(one),
             "qmap3=MAP1": "qmap3=" + str(one), "qmap3=BAD": "qmap3=" + str(bad),
             "qmap3=MISSING": "qmap3=" + str(tmp_path / "none.txt")}
    argv = [names.get(a, a) for a in args]
    clean = {k: v for k, v in os.environ.items() if not k.startswith("DCT3D_CODEC_")}
    r = subprocess.run([pkg.CLI_PATH] + argv, capture_output=True, text=True,
                       env=dict(clean, **{k: names.get(v, v) for k, v in env.items()}))
    assert r.returncode == 1 and said in r.stdout, r.stdout
    assert not out.exists() and not any((tmp_path / ("out.bin" + s)).exists() for s in (".red", ".green", ".blue"))
    assert good.read_text() == "5 12 12\n12 16 16\n" and one.read_text() == "5\n12\n"
