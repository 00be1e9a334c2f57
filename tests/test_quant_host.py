"""CPU: the codec host's side of quantiser tables -- the one parser of a quantiser given as text
(codec_parse_quant: the CLI's argument and DCT3D_CODEC_QUANT) and the reference-signature helpers' _steps
siblings (cube_io.c), against the reference's own C helpers (oracle/_ref) for the reference table."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from test_host_codec import _ref_or_skip


@pytest.fixture(scope="module")
def codec(pkg):
    L = C.CDLL(pkg.CODEC_LIB_PATH)
    L.codec_parse_quant.argtypes = [C.c_char_p, C.c_int, C.c_void_p]
    L.codec_set_quant.argtypes = [C.c_char_p]
    for name in ("applyQuantization_steps", "applyDequantization_steps"):
        getattr(L, name).argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    for name in ("applyQuantization_d", "applyDequantization_d"):
        getattr(L, name).argtypes = [C.c_void_p, C.c_size_t, C.c_int]
    return L


def _parse(codec, text, depth):
    steps = np.full(32, -1, np.int32)
    rc = codec.codec_parse_quant(text.encode() if text is not None else None, depth, steps.ctypes.data)
    assert rc in (0, 1)
    if rc:
        assert (steps == -1).all(), "a refused text leaves the steps untouched"
        return None
    assert (steps[depth + 14:] == -1).all(), "exactly depth + 14 steps are written"
    return steps[:depth + 14].tolist()


@pytest.mark.parametrize("depth", [8, 4])
def test_parse_quant_accepts(codec, pkg, depth):
    n = depth + 14
    for q in (0, 1, 2, 5, 12, 30, 255):
        assert _parse(codec, f"q={q}", depth) == pkg.quant_table(q, depth).tolist()
    assert _parse(codec, "q=5", depth) == [max(1, 5 * s) for s in range(n)]
    lst = [(37 * s) % 255 + 1 for s in range(n)]
    assert _parse(codec, ",".join(map(str, lst)), depth) == lst
    assert _parse(codec, ",".join(["255"] * n), depth) == [255] * n
    assert _parse(codec, ",".join(["1"] * n), depth) == [1] * n
    assert _parse(codec, "q=005", depth) == pkg.quant_table(5, depth).tolist()


@pytest.mark.parametrize("depth", [8, 4])
def test_parse_quant_rejects(codec, depth):
    n = depth + 14
    ones = ["1"] * n
    bad = ["", "q", "q=", "q=-1", "q=+5", "q= 5", "q=256", "q=5x", "q=5,", "Q=5", "5", "q=1.5",
           ",".join(ones[:-1]), ",".join(ones + ["1"]), ",".join(ones) + ",", "," + ",".join(ones),
           ",".join(["0"] + ones[1:]), ",".join(ones[:-1] + ["256"]), ",".join(ones[:3] + ["-4"] + ones[4:]),
           ",".join(ones[:3] + [""] + ones[4:]), ",".join(ones[:3] + [" 7"] + ones[4:]), ";".join(ones),
           ",".join(ones[:3] + ["7x"] + ones[4:]), ",".join(["99999999999999999999"] + ones[1:])]
    for text in bad:
        assert _parse(codec, text, depth) is None, repr(text)
    assert _parse(codec, None, depth) is None
    other = 4 if depth == 8 else 8
    assert _parse(codec, ",".join(["1"] * (other + 14)), depth) is None  # the other depth's length
    assert _parse(codec, "q=5", 5) is None and _parse(codec, "q=5", 0) is None
    assert codec.codec_parse_quant(b"q=5", depth, None) == 1


def test_cli_rejects_a_bad_quantiser_without_a_device(pkg, tmp_path):
    src = tmp_path / "in.raw"
    src.write_bytes(bytes(64 * 64 * 8))
    for bad in ("q=300", "1,2,3", "fine"):
        r = subprocess.run([pkg.CLI_PATH, "encode", str(src), str(tmp_path / "x.bin"), "64", "64", "8", "1", "8", bad],
                           capture_output=True, text=True)
        assert r.returncode == 1 and "Invalid quantiser" in r.stdout, r.stdout
        assert not (tmp_path / "x.bin").exists()
    r = subprocess.run([pkg.CLI_PATH], capture_output=True, text=True)
    assert "q=<int>" in r.stdout


def _steps_cube(T, depth):
    z, y, x = np.ogrid[:depth, :8, :8]
    return np.asarray(T, np.float64)[x + y + z]


@pytest.mark.parametrize("depth", [8, 4])
def test_steps_helpers(codec, pkg, oracle, depth):
    """a 16 x 16 x depth block (4 cubes) of DCT coefficients: the reference table through the _steps helpers is
    the _d helpers bit for bit; any table is C's round(c / step), round(c * step) in double, back to float"""
    fr = pkg.synthetic.frames(16, 16, depth, kind="uniform")
    dct = oracle.to_cubes(oracle.Plan(8, 8, depth).dct(fr), 8, 8, depth).astype(np.float32)
    ref_t = pkg.quant_table(5, depth)
    for fn in ("applyQuantization", "applyDequantization"):
        a, b = dct.copy().reshape(-1), dct.copy().reshape(-1)
        getattr(codec, fn + "_d")(a.ctypes.data, a.size, depth)
        getattr(codec, fn + "_steps")(b.ctypes.data, b.size, depth, ref_t.ctypes.data)
        assert np.array_equal(a, b), fn
    rnd = np.random.default_rng(3).integers(1, 256, depth + 14).astype(np.int32)
    for T in (pkg.quant_table(12, depth), rnd):
        st = _steps_cube(T, depth)
        v = dct.astype(np.float64)
        a = dct.copy().reshape(-1)
        codec.applyQuantization_steps(a.ctypes.data, a.size, depth, T.ctypes.data)
        x = v / st
        want = (np.sign(x) * np.floor(np.abs(x) + 0.5)).astype(np.float32)  # C round(): half away from zero
        assert np.array_equal(a.reshape(dct.shape), want)
        b = want.copy().reshape(-1)
        codec.applyDequantization_steps(b.ctypes.data, b.size, depth, T.ctypes.data)
        assert np.array_equal(b.reshape(dct.shape), (want.astype(np.float64) * st).astype(np.float32))


def test_steps_helpers_equal_the_reference_helpers(codec, pkg, oracle):
    """applyQuantization_steps / applyDequantization_steps with the reference table against the reference's own
    applyQuantization / applyDequantization (oracle/_ref, block depth 8) on a 16 x 16 x 8 block"""
    R = _ref_or_skip()
    fr = pkg.synthetic.frames(16, 16, 8, kind="uniform")
    dct = oracle.to_cubes(oracle.Plan(8, 8, 8).dct(fr)).astype(np.float32).reshape(-1)
    ref_t = pkg.quant_table(5, 8)
    for fn in ("applyQuantization", "applyDequantization"):
        a, b = dct.copy(), dct.copy()
        getattr(R, fn).argtypes = [C.c_void_p, C.c_size_t]
        getattr(R, fn)(a.ctypes.data, a.size)
        getattr(codec, fn + "_steps")(b.ctypes.data, b.size, 8, ref_t.ctypes.data)
        assert np.array_equal(a, b), fn
