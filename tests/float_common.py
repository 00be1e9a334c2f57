"""Shared by test_float_ref.py (CPU) and test_gpu_float.py (GPU): the two references the float kernels are held to,
and the inputs both modules use.

  * dct_ref: a separable orthonormal DCT-II / DCT-III in numpy long double, built from the cosine definition
    (M[k][n] = s_k cos(pi (2 n + 1) k / 2 N), s_0 = sqrt(1 / N), s_k = sqrt(2 / N)); cubes are [z][y][x].  It shares
    nothing with the kernels, the butterflies or the oracle.
  * emu_cube_f32 / emu_fwd64: tests/native/emulate_float.cpp, the arithmetic of cube_f32_kernel and
    fwd64_raster_kernel restated on the host from csrc/dct_butterfly.h, built as cert_common._libs() builds its
    libraries (g++ -O2 -ffp-contract=off -fno-fast-math).  With contraction off on both sides and one butterfly source,
    IEEE fp64 arithmetic is deterministic: the device's outputs must equal the emulation's bit for bit.

No GPU is needed by anything in this module."""
import atexit
import ctypes as C
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

import cert_common as cc
import quant_common as qc

LD = np.longdouble
REL = 1e-9  # DESIGN "Float outputs": |err| <= 1e-9 max(1, |ref|) before the final rounding


# ---- the long-double reference --------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def dct_matrix(N):
    """long double [k][n]: the orthonormal DCT-II matrix of N points"""
    pi = 4 * np.arctan(LD(1))
    k, n = np.ogrid[:N, :N]
    m = np.cos(pi * ((2 * n + 1) * k).astype(LD) / LD(2 * N)) * np.sqrt(LD(2) / LD(N))
    m[0] = np.sqrt(LD(1) / LD(N))
    m.setflags(write=False)
    return m


def dct_ref(cubes, depth, inverse):
    """[n, depth, 8, 8] of any real type -> float64, the same shape: the separable DCT-II (inverse: DCT-III, its
    transpose) along x, y and z, accumulated in long double; no clamp"""
    v = np.asarray(cubes).astype(LD).reshape(-1, depth, 8, 8)
    m8, md = dct_matrix(8), dct_matrix(depth)
    if inverse:
        m8, md = m8.T, md.T
    v = np.einsum("kx,nzyx->nzyk", m8, v)
    v = np.einsum("ky,nzyx->nzkx", m8, v)
    v = np.einsum("kz,nzyx->nkyx", md, v)
    return v.astype(np.float64)


def tol(ref):
    """the project's bound on a float output before its final rounding"""
    return REL * np.maximum(1.0, np.abs(ref))


def f32_window(ref):
    """(lo, hi) float32: the roundings to nearest of ref - tol and ref + tol.  Rounding is monotone, so lo <= out <= hi
    says exactly that out is the float rounding of a value within tol of ref"""
    e = tol(ref)
    return (ref - e).astype(np.float32), (ref + e).astype(np.float32)


def in_f32_window(out, ref):
    lo, hi = f32_window(ref)
    return bool(np.all((lo <= out) & (out <= hi)))


# ---- the emulation ----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _lib():
    d = tempfile.mkdtemp(prefix="float_emu_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    so = os.path.join(d, "emulate_float.so")
    subprocess.run(cc.GXX + [os.path.join(cc.NATIVE, "emulate_float.cpp"), "-o", so], check=True)
    L = C.CDLL(so)
    L.emulate_cube_f32.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.emulate_fwd64.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_void_p]
    return L


def emu_cube_f32(cubes, depth, inverse, order=0, want_pre=False):
    """cube_f32_kernel<depth, inverse> on float32 cubes [n, depth, 8, 8] -> float32, the same shape (want_pre: and the
    fp64 values before the clamp and the cast).  order = 1 runs the passes X, Y, Z instead of the kernel's Y, X, Z:
    another summation order of the same transform, for the check that the equality sees what the tolerance cannot."""
    x = np.ascontiguousarray(cubes, np.float32).reshape(-1, depth, 8, 8)
    out = np.empty_like(x)
    pre = np.empty(x.shape, np.float64) if want_pre else None
    rc = _lib().emulate_cube_f32(x.ctypes.data, x.shape[0], depth, int(inverse), order, out.ctypes.data,
                                 pre.ctypes.data if want_pre else None)
    assert rc == 0
    return (out, pre) if want_pre else out


def emu_fwd64(cubes, depth, order=0):
    """fwd64_raster_kernel<depth> on the uint8 cubes of a raster [n, depth, 8, 8] -> float64, the same shape.
    order = 1: the passes X, Y, Z instead of the kernel's X, Z, Y (as for emu_cube_f32)"""
    x = np.ascontiguousarray(cubes, np.uint8).reshape(-1, depth, 8, 8)
    out = np.empty(x.shape, np.float64)
    assert _lib().emulate_fwd64(x.ctypes.data, x.shape[0], depth, order, out.ctypes.data) == 0
    return out


# ---- inputs of cube_f32_kernel ----------------------------------------------------------------------------------------

def cpw(depth):
    """cubes per wave of cube_f32_kernel (the decode's geometry)"""
    return 4 if depth == 8 else 8


def tile(depth):
    """cubes per block: 4 waves"""
    return 4 * cpw(depth)


def tail_counts(depth):
    """1, 2, 8, 9, 16 and 18 blocks, with and without a partial wave: a grid that is a multiple of 8 blocks takes
    xcd_tile()'s first arm throughout (at 16 blocks with a stride of 2), every other grid its second arm for the
    blocks past the last multiple of 8"""
    c, t = cpw(depth), tile(depth)
    return [1, c - 1, c, c + 1, t - 1, t + 1, 7 * t + 1, 8 * t, 8 * t + 1, 9 * t - 1, 15 * t + c + 1, 17 * t + c + 1]


def _frames(w, h, stacks, depth, kind, frame0=7):
    return qc.pkg().synthetic.frames(w, h, stacks * depth, frame0=frame0, kind=kind)


def _pixel_cubes(w, h, stacks, depth, kind, frame0=7):
    import oracle
    return oracle.to_cubes(_frames(w, h, stacks, depth, kind, frame0), 8, 8, depth)


def _dequantised_cubes(w, h, stacks, depth, kind, frame0=7):
    """the reference decoder's input: the oracle's quantised coefficients of the frames, dequantised"""
    import oracle
    fr = _frames(w, h, stacks, depth, kind, frame0)
    q = qc.plan(depth).encode_q(fr)
    return oracle.to_cubes(oracle.dequantize(q, w, h, fr.shape[0], 8, 8, depth), 8, 8, depth)


def _impulses(depth, amplitude):
    n = 64 * depth
    x = np.zeros((n, n), np.float64)
    x[np.arange(n), np.arange(n)] = amplitude
    return x.reshape(n, depth, 8, 8)


def _content_stacks(depth):
    return 3 if depth == 8 else 5


def _build(name, depth, inverse):
    rng = np.random.default_rng([20261020, depth, int(inverse)])
    dc = np.sqrt(64.0 * depth)
    if name in ("uniform", "ramp"):  # 24 x 16: 6 cubes per stack, 18 or 30 cubes: a partial block, a partial wave
        f = _dequantised_cubes if inverse else _pixel_cubes
        return f(24, 16, _content_stacks(depth), depth, name)
    if name == "frame64x32":  # the shapes of the drop-in tests this module replaced: 64 x 32 x 8, one stack at 8x8x8
        f = _dequantised_cubes if inverse else _pixel_cubes
        return f(64, 32, 1, depth, "ramp" if inverse else "uniform", frame0=0)
    if name == "pool":  # the tail cases take its first n cubes; the inverse's range -20 .. 286 reaches both clamp arms
        px = rng.integers(0, 256, size=(max(tail_counts(depth)), depth, 8, 8)).astype(np.float64)
        return dct_ref(px * 1.2 - 20.0, depth, False) if inverse else px
    if not inverse:
        if name in ("basis255", "basis-1000.5"):  # every position alone, then cubes that leave the last tile partial
            tail = rng.integers(0, 256, size=(3 if depth == 8 else 5, depth, 8, 8)).astype(np.float64)
            return np.concatenate([_impulses(depth, 255.0 if name == "basis255" else -1000.5), tail])
        if name == "gauss":
            return rng.normal(0.0, 100.0, size=(37, depth, 8, 8))
    else:
        if name == "basis":  # mid-grey plus every coefficient alone: the pixels stay inside (0, 255)
            x = _impulses(depth, 100.0)
            x[:, 0, 0, 0] += 128.0 * dc
            return x
        if name == "const":  # constant cubes at, inside and outside the clamp's ends
            x = np.zeros((5, depth, 8, 8), np.float64)
            x[:, 0, 0, 0] = np.array([0.0, 255.0, -3.0, 300.0, 254.5]) * dc
            return x
    raise KeyError((name, depth, inverse))


FORWARD = ("basis255", "basis-1000.5", "uniform", "ramp", "gauss", "pool")
INVERSE = ("basis", "uniform", "ramp", "const", "pool")
# the inputs whose values are pixels (forward) or the coefficients of pixel-range cubes (inverse): DESIGN's measured
# error is the largest over these
PIXEL_RANGE = {False: ("basis255", "uniform", "ramp", "pool"), True: ("basis", "uniform", "ramp", "const", "pool")}


def case_names(depth, inverse):
    return (INVERSE if inverse else FORWARD) + (("frame64x32",) if depth == 8 else ())


class F32Case:
    """x: the float32 input [n, depth, 8, 8]; ref: dct_ref of x (float64, no clamp); emu: the emulation's float32
    output; all read-only"""

    def __init__(self, name, depth, inverse):
        self.name, self.depth, self.inverse = name, depth, inverse
        self.x = np.ascontiguousarray(_build(name, depth, inverse), np.float32)
        self.ref = dct_ref(self.x, depth, inverse)
        self.emu = emu_cube_f32(self.x, depth, inverse)
        for a in (self.x, self.ref, self.emu):
            a.setflags(write=False)

    @property
    def n(self):
        return self.x.shape[0]

    def expected(self):
        """what the output is held to by the window: ref, clipped to [0, 255] for the inverse (clipping is
        1-Lipschitz, so a value within tol of ref clips to a value within tol of this)"""
        return np.clip(self.ref, 0.0, 255.0) if self.inverse else self.ref


@functools.lru_cache(maxsize=None)
def f32_case(name, depth, inverse):
    return F32Case(name, depth, bool(inverse))


# ---- inputs of fwd64_raster_kernel ------------------------------------------------------------------------------------

# (w, h, stacks): a single cube; nbx odd and a partial block (30 cubes); one cube into a second block (33); several
# blocks and a partial last one (135); 512 cubes with one pixel each
RASTER_SHAPES = ((8, 8, 1), (24, 16, 5), (264, 8, 1), (72, 40, 3), (64, 64, 8))


class RasterCase:
    """frames: uint8 [stacks depth, h, w]; cubes: its cubes in the calls' order; emu: the emulation's fp64 output;
    ref: dct_ref of the cubes; all read-only"""

    def __init__(self, w, h, stacks, depth):
        import oracle
        self.w, self.h, self.stacks, self.depth = w, h, stacks, depth
        if (w, h, stacks) == (64, 64, 8):  # cube i: 255 at position i of the cube (8x8x4: i mod 256), 0 elsewhere
            cubes = np.zeros((512, 64 * depth), np.uint8)
            cubes[np.arange(512), np.arange(512) % (64 * depth)] = 255
            self.frames = oracle.from_cubes(cubes.reshape(512, depth, 8, 8), w, h, stacks * depth)
        else:
            self.frames = _frames(w, h, stacks, depth, "uniform", frame0=11)
        self.frames = np.ascontiguousarray(self.frames, np.uint8)
        self.cubes = oracle.to_cubes(self.frames, 8, 8, depth)
        self.emu = emu_fwd64(self.cubes, depth)
        self.ref = dct_ref(self.cubes, depth, False)
        for a in (self.frames, self.cubes, self.emu, self.ref):
            a.setflags(write=False)

    @property
    def n(self):
        return self.cubes.shape[0]

    def oracle_dct(self):
        """Plan.dct, the Java-semantics fold, as cubes"""
        import oracle
        return oracle.to_cubes(qc.plan(self.depth).dct(self.frames), 8, 8, self.depth)


@functools.lru_cache(maxsize=None)
def raster_case(w, h, stacks, depth):
    return RasterCase(w, h, stacks, depth)
