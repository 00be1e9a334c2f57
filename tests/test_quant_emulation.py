"""CPU: certify-or-replay with quantiser tables, through the host emulations of the kernels' arithmetic.

Encode: tests/native/emulate_encode.cpp unchanged -- it takes {1 / step, G, E} as arguments -- fed each table T's
plan tables (dct3d_plan_query_quant), over test_emulation.py's input families.  Soundness: every AC coefficient
the emulated kernel does NOT flag equals the reference (quant_common.py: the oracle's Java DCT, then the numpy
definition of the quantiser); the flagged ones are the device's exact paths' (test_gpu_quant.py).  There is no
cap on the flag rate here: small steps legitimately flag more.  The DC never goes through the fp32 path: its
closed form JavaRound(S * coef_dc / step[0]) is compared on its own.

Decode: tests/native/emulate_decode_quant.cpp (emulate_decode.cpp with the table) against Java's InverseDCT fold
of the dequantised cubes: |v - v_java| <= dec_G * L1 + dec_E with L1 = sum |q * step|, the certificate's margin,
for the cubes the kernel certifies at all (L1 < dec_l1_max)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import quant_common as qc
from test_emulation import SRC, _inputs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "3ddctvideoencoding_amd", "csrc")
GXX = ["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-std=c++17", "-shared", "-fPIC", "-I", CSRC]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    out = tmp_path_factory.mktemp("emuq") / "libemu.so"
    subprocess.run(GXX + [SRC, "-o", str(out)], check=True)
    L = C.CDLL(str(out))
    L.emulate_encode.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def emu_dec(tmp_path_factory):
    out = tmp_path_factory.mktemp("emudq") / "libemudq.so"
    subprocess.run(GXX + [os.path.join(REPO, "tests", "native", "emulate_decode_quant.cpp"), "-o", str(out)], check=True)
    L = C.CDLL(str(out))
    L.emulate_decode_quant.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


@functools.lru_cache(maxsize=None)
def _cases(depth):
    """per input family: (cubes u8 [n, depth, 8, 8], the oracle's fp64 DCT in the same layout), computed once"""
    import oracle
    out = []
    for fr in _inputs(qc.pkg(), depth):
        cubes = oracle.to_cubes(fr, 8, 8, depth)
        dct = oracle.to_cubes(qc.plan(depth).dct(fr), 8, 8, depth)
        cubes.setflags(write=False)
        dct.setflags(write=False)
        out.append((cubes, dct))
    return out


def _run(emu, p, cubes, depth):
    cubes = np.ascontiguousarray(cubes, np.uint8)
    n = cubes.shape[0]
    q = np.empty(cubes.size, np.int32)
    fl = np.empty(cubes.size, np.uint8)
    val = np.empty(cubes.size, np.float32)
    A = np.empty(n, np.float32)
    t = [np.ascontiguousarray(p[k], np.float32) for k in ("enc_rstep", "enc_G", "enc_E")]
    emu.emulate_encode(cubes.ctypes.data, n, depth, t[0].ctypes.data, t[1].ctypes.data, t[2].ctypes.data,
                       p["coef_dc"], q.ctypes.data, fl.ctypes.data, val.ctypes.data, A.ctypes.data)
    shape = (n, depth, 8, 8)
    return q.reshape(shape), fl.reshape(shape).astype(bool), val.reshape(shape), A


@pytest.mark.parametrize("name", qc.TABLE_NAMES)
@pytest.mark.parametrize("depth", [8, 4])
def test_unflagged_coefficients_equal_reference(emu, pkg, depth, name):
    T = qc.tables(depth)[name]
    p = pkg.plan_query(8, 8, depth, steps=T)
    step = T[np.add.outer(np.add.outer(np.arange(depth), np.arange(8)), np.arange(8))].astype(np.float64)
    K = p["enc_K"].reshape(depth, 8, 8)
    n_open = n_all = 0
    for cubes, dct in _cases(depth):
        q, fl, val, A = _run(emu, p, cubes, depth)
        ref = pkg.quantize_ref(dct, T)
        ac = np.ones(q.shape, bool)
        ac[:, 0, 0, 0] = False
        bad = (q != ref) & ~fl & ac
        assert not bad.any(), f"{bad.sum()} uncertified mismatches"
        assert not fl[:, 0, 0, 0].any()  # the DC is never flagged
        # the per-coefficient bound on the quotient: A K / step + 1e-9
        err = np.abs(val.astype(np.float64) - dct) / step
        err[:, 0, 0, 0] = 0.0
        assert (err <= A[:, None, None, None].astype(np.float64) * K[None] / step + 1e-9).all()
        # the DC by its closed form: the Java fold of the single DC group is S * coef_dc (one product), then
        # the division by step[0] and Math.round
        S = cubes.reshape(cubes.shape[0], -1).astype(np.int64).sum(axis=1).astype(np.float64)
        assert np.array_equal(S * p["coef_dc"], dct[:, 0, 0, 0])
        dc = (S * p["coef_dc"]) / float(T[0])
        f = np.floor(dc)
        assert np.array_equal((f + (dc - f >= 0.5)).astype(np.int32), ref[:, 0, 0, 0])
        n_open += int(fl.sum())
        n_all += fl.size
    print(f"8x8x{depth} {name}: {n_open} of {n_all} coefficients open ({n_open / n_all:.2e})")  # a figure, no condition


@pytest.mark.parametrize("name", qc.TABLE_NAMES)
@pytest.mark.parametrize("depth", [8, 4])
def test_decode_bound_dominates_observed_error(emu_dec, pkg, oracle, depth, name):
    T = qc.tables(depth)[name]
    p = pkg.plan_query(8, 8, depth, steps=T)
    W, H, F = 64, 32, depth * 2
    rng = np.random.default_rng(99)
    step = T[np.add.outer(np.add.outer(np.arange(depth), np.arange(8)), np.arange(8))].astype(np.float64)
    n = (F // depth) * (H // 8) * (W // 8)
    qs = [pkg.quantize_ref(dct[:n], T) for _, dct in _cases(depth)]  # (cubes are independent: the first n of each)
    # random cubes whose dequantised values are a few hundred at most, and sparse +-150 spikes
    qs.append(np.rint(rng.uniform(-200, 200, (n, depth, 8, 8)) / step).astype(np.int32))
    qs.append((rng.integers(-1, 2, (n, depth, 8, 8)) * np.rint(150 / step)).astype(np.int32))
    worst, n_cert = 0.0, 0
    for q in qs:
        q = np.ascontiguousarray(q, np.int32)
        Tc = np.ascontiguousarray(T, np.int32)
        v = np.empty(q.size, np.float64)
        l1 = np.empty(n, np.float64)
        emu_dec.emulate_decode_quant(q.ctypes.data, n, depth, Tc.ctypes.data, v.ctypes.data, l1.ctypes.data)
        v = v.reshape(n, depth, 8, 8)
        assert np.array_equal(l1, np.abs(pkg.dequantize_ref(q, T)).reshape(n, -1).sum(axis=1))  # exact integers
        java = oracle.to_cubes(qc.plan(depth).idct(oracle.from_cubes(pkg.dequantize_ref(q, T), W, H, F)), 8, 8, depth)
        cert = l1 < p["dec_l1_max"]  # the others go to the exact replay whatever their values
        err = np.abs(np.clip(v, 0.0, 255.0) - java)[cert]
        bound = (l1[:, None, None, None] * p["dec_G"] + p["dec_E"])[cert]
        assert (err <= bound).all()
        if cert.any():
            worst = max(worst, float((err / bound).max()))
            assert (np.abs(v[cert]) <= l1[cert][:, None, None, None] * (32000.0 / p["dec_l1_max"]) * (1 + 1e-6) + 1e-6).all()
        n_cert += int(cert.sum())
    assert n_cert > 0 and worst < 1.0
