"""3ddctvideoencoding_amd -- MI355X-native 3D-DCT hot path of julianopiccoli/3dDCTVideoEncoding.

The product is the C-ABI library ``lib/libdct3d.so`` (HIP kernels for gfx950 + runtime, declared in
``include/dct3d.h``) and the reference-compatible C codec host ``lib/libdct3dcodec.so`` /
``lib/dct3d_codec``.  This module is a thin ctypes binding with the same entry-point names; it has
NO fallback: if the library is missing or no HIP device is present the calls raise.

Since the package name starts with a digit, import it with
``importlib.import_module("3ddctvideoencoding_amd")``.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Optional

import numpy as np

from . import synthetic  # noqa: F401  (integer-only generator shared with the device kernel)

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(PKG_DIR, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libdct3d.so")
DIAG_LIB_PATH = os.path.join(LIB_DIR, "libdct3d_diag.so")  # measurement / test support (include/dct3d_diag.h)
CODEC_LIB_PATH = os.path.join(LIB_DIR, "libdct3dcodec.so")
CLI_PATH = os.path.join(LIB_DIR, "dct3d_codec")
REPO_DIR = os.path.dirname(PKG_DIR)
INCLUDE_DIR = os.path.join(REPO_DIR, "include")

DCT3D_OK, DCT3D_EINVAL, DCT3D_EDEVICE, DCT3D_ENOMEM, DCT3D_EKERNEL, DCT3D_ENOSPC, DCT3D_ENODATA = 0, 1, 2, 3, 4, 5, 6
# test / diagnostic options (include/dct3d.h, Context.set_option)
DCT3D_OPT_DEC_MARGIN, DCT3D_OPT_ENC_NO_RECHECK, DCT3D_OPT_EG_TWO_STEP, DCT3D_OPT_EG_NO_RESOLVE = 2, 3, 5, 6
DCT3D_OPT_EG_FORCE_RETRY = 8
DCT3D_OPT_EG_DEC_GROUPS = 9
DCT3D_OPT_EG_FUSED_FRONT = 10
DCT3D_OPT_QUANT_FORCE_TABLE = 11
# the colour transform of the packed RGB24 stream calls and the rate probe (dct3d.h; rgb_to_ycbcr below)
DCT3D_OPT_COLOUR = 12
DCT3D_COLOUR_PLANES, DCT3D_COLOUR_YCBCR = 0, 1
# 4:2:0 chroma subsampling on top of the colour transform (dct3d.h; Context.set_chroma, rgb_to_ycbcr420 below)
DCT3D_CHROMA_444, DCT3D_CHROMA_420 = 0, 1
# bytes of decoded planes the RGB-domain distortion probe keeps per range of stacks (dct3d.h; or one stack's)
DCT3D_RGB_PLANE_BUDGET = 64 << 20
# bytes of 4 x 4 block records the SSIM probe keeps per range of stacks (dct3d.h; or one stack's): per stack and
# channel D ceil(w / 4) ceil(h / 4) (8 n_tables + 4)
DCT3D_SSIM_BLOCK_BUDGET = 16 << 20

# Every symbol include/dct3d.h declares (checked by tests/test_abi.py).
ABI_SYMBOLS = (
    "dct3d_abi_version", "dct3d_strerror", "dct3d_ctx_create", "dct3d_ctx_destroy",
    "dct3d_ctx_set_stream", "dct3d_ctx_info", "dct3d_ctx_set_option", "dct3d_ctx_set_profiling", "dct3d_synchronize", "dct3d_get_stats",
    "dct3d_reset_timers",
    "dct3d_encode_stacks", "dct3d_encode_stacks_dev", "dct3d_decode_stacks", "dct3d_decode_stacks_dev",
    "dct3d_forward_f32", "dct3d_inverse_f32", "dct3d_forward_f32_dev", "dct3d_inverse_f32_dev",
    "dct3d_plan_query",
    "dct3d_eg_encode_dev", "dct3d_encode_eg", "dct3d_eg_fetch", "dct3d_diagonal_order",
    "dct3d_eg_decode_dev", "dct3d_decode_eg", "dct3d_encode_eg_dev", "dct3d_decode_eg_dev",
    "dct3d_encode_stacks_rgb", "dct3d_encode_stacks_rgb_dev", "dct3d_decode_stacks_rgb", "dct3d_decode_stacks_rgb_dev",
    "dct3d_encode_frames", "dct3d_encode_frames_dev", "dct3d_decode_frames", "dct3d_decode_frames_dev",
    "dct3d_encode_eg_frames", "dct3d_encode_eg_frames_dev", "dct3d_eg_fetch_channel",
    "dct3d_decode_eg_frames", "dct3d_decode_eg_frames_dev",
    "dct3d_ctx_set_quant", "dct3d_ctx_get_quant", "dct3d_plan_query_quant",
    "dct3d_rate_frames", "dct3d_rate_frames_dev",
    "dct3d_distortion_frames", "dct3d_distortion_frames_dev",
    "dct3d_encode_eg_frames_vq", "dct3d_encode_eg_frames_vq_dev",
    "dct3d_decode_eg_frames_vq", "dct3d_decode_eg_frames_vq_dev",
    "dct3d_ctx_set_chroma", "dct3d_ctx_get_chroma", "dct3d_chroma_size",
    "dct3d_encode_eg_frames_vqc", "dct3d_encode_eg_frames_vqc_dev",
    "dct3d_decode_eg_frames_vqc", "dct3d_decode_eg_frames_vqc_dev",
    "dct3d_distortion_rgb_frames", "dct3d_distortion_rgb_frames_dev",
    "dct3d_ssim_frames", "dct3d_ssim_frames_dev", "dct3d_ssim_windows",
    "dct3d_ssim_rgb_frames", "dct3d_ssim_rgb_frames_dev",
    "dct3d_eg_sync_launches",
)
# Every symbol include/dct3d_diag.h declares (libdct3d_diag.so; none of them is in libdct3d.so).
DIAG_SYMBOLS = ("dct3d_fill_synthetic_dev", "dct3d_bandwidth_probe_dev", "dct3d_encode_memonly_dev",
                "dct3d_encode_diag_dev", "dct3d_encode_trace_dev", "dct3d_encode_strip_dev", "dct3d_decode_diag_dev")


class Dct3dError(RuntimeError):
    def __init__(self, code: int, what: str):
        super().__init__(f"{what}: {strerror(code)} ({code})")
        self.code = code


class PlanInfo(C.Structure):
    _fields_ = [("cube_size", C.c_int), ("n_mults", C.c_int), ("treeified", C.c_int), ("coef_dc", C.c_double),
                ("dec_G", C.c_double), ("dec_E", C.c_double), ("enc_rstep", C.c_float * 32),
                ("enc_G", C.c_float * 32), ("enc_E", C.c_float * 32), ("enc_thr64", C.c_double * 32),
                ("dec_l1_max", C.c_float)]


class Stats(C.Structure):
    _fields_ = [("n_units", C.c_uint64), ("n_flagged", C.c_uint64),
                ("n_timed", C.c_uint64), ("kernel_ms_total", C.c_double), ("aux_ms_total", C.c_double),
                ("n_rechecked", C.c_uint64)]

    def as_dict(self) -> dict:
        return {f: getattr(self, f) for f, _ in self._fields_}


_lib = None


def lib() -> C.CDLL:
    """Load libdct3d.so (raises if it has not been built: run __graft_entry__.build() / make)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: build it with `make` (or __graft_entry__.build())")
        # PyTorch-ROCm bundles its own libamdhip64 (SONAME libamdhip64.so.7).  If libdct3d.so were
        # loaded first, torch would later load a second HIP runtime and find no GPU; loading torch
        # first lets libdct3d.so bind to the already-loaded runtime (one HIP runtime per process).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        vp, i32, sz, u64, i64 = C.c_void_p, C.c_int, C.c_size_t, C.c_uint64, C.c_int64
        L.dct3d_abi_version.restype = i32
        L.dct3d_strerror.restype = C.c_char_p
        L.dct3d_strerror.argtypes = [i32]
        L.dct3d_ctx_create.argtypes = [i32, i32, i32, i32, C.POINTER(vp)]
        L.dct3d_ctx_destroy.argtypes = [vp]
        L.dct3d_ctx_destroy.restype = None
        L.dct3d_ctx_set_stream.argtypes = [vp, vp]
        L.dct3d_ctx_set_profiling.argtypes = [vp, i32]
        L.dct3d_ctx_set_option.argtypes = [vp, i32, C.c_double]
        L.dct3d_synchronize.argtypes = [vp]
        L.dct3d_get_stats.argtypes = [vp, C.POINTER(Stats)]
        L.dct3d_reset_timers.argtypes = [vp]
        for name in ("dct3d_encode_stacks", "dct3d_encode_stacks_dev"):
            getattr(L, name).argtypes = [vp, vp, i32, i32, i32, vp, vp]
        for name in ("dct3d_decode_stacks", "dct3d_decode_stacks_dev"):
            getattr(L, name).argtypes = [vp, vp, i32, i32, i32, vp]
        for name in ("dct3d_encode_stacks_rgb", "dct3d_encode_stacks_rgb_dev", "dct3d_decode_stacks_rgb",
                     "dct3d_decode_stacks_rgb_dev"):
            getattr(L, name).argtypes = [vp, vp, i32, i32, i32, vp]
        for name in ("dct3d_encode_frames", "dct3d_encode_frames_dev", "dct3d_decode_frames", "dct3d_decode_frames_dev"):
            getattr(L, name).argtypes = [vp, vp, i32, i32, i32, i32, vp]
        for name in ("dct3d_forward_f32", "dct3d_inverse_f32", "dct3d_forward_f32_dev", "dct3d_inverse_f32_dev"):
            getattr(L, name).argtypes = [vp, vp, sz, vp]
        L.dct3d_ctx_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(vp)]
        L.dct3d_plan_query.argtypes = [i32, i32, i32, C.POINTER(PlanInfo), vp, vp, vp, vp]
        L.dct3d_plan_query_quant.argtypes = [i32, i32, i32, vp, i32, C.POINTER(PlanInfo), vp, vp, vp, vp]
        L.dct3d_ctx_set_quant.argtypes = [vp, vp, i32]
        L.dct3d_ctx_get_quant.argtypes = [vp, vp, i32]
        L.dct3d_eg_encode_dev.argtypes = [vp, vp, u64, C.c_uint8, i32, vp, u64, C.POINTER(u64)]
        L.dct3d_encode_eg.argtypes = [vp, vp, i32, i32, i32, C.c_uint8, i32, C.POINTER(u64)]
        L.dct3d_encode_eg_dev.argtypes = [vp, vp, i32, i32, i32, C.c_uint8, i32, vp, u64, C.POINTER(u64)]
        L.dct3d_eg_fetch.argtypes = [vp, vp, u64]
        L.dct3d_diagonal_order.argtypes = [i32, i32, i32, vp]
        L.dct3d_eg_decode_dev.argtypes = [vp, vp, u64, u64, u64, vp, C.POINTER(u64)]
        L.dct3d_decode_eg.argtypes = [vp, vp, u64, i32, i32, i32, i32, vp, C.POINTER(u64)]
        L.dct3d_decode_eg_dev.argtypes = [vp, vp, u64, u64, i32, i32, i32, vp, C.POINTER(u64)]
        L.dct3d_eg_sync_launches.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
        # (the per-channel arrays as plain addresses: ctypes arrays convert, None is NULL)
        L.dct3d_encode_eg_frames_dev.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp]
        L.dct3d_encode_eg_frames.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, vp]
        L.dct3d_eg_fetch_channel.argtypes = [vp, i32, vp, u64]
        L.dct3d_decode_eg_frames_dev.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp]
        L.dct3d_decode_eg_frames.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp]
        L.dct3d_rate_frames_dev.argtypes = [vp, vp, i32, i32, i32, i32, vp, i32, vp, vp]
        L.dct3d_rate_frames.argtypes = [vp, vp, i32, i32, i32, i32, vp, i32, vp]
        L.dct3d_distortion_frames_dev.argtypes = [vp, vp, i32, i32, i32, i32, vp, i32, vp, vp, vp]
        L.dct3d_distortion_frames.argtypes = [vp, vp, i32, i32, i32, i32, vp, i32, vp, vp]
        # (the base stream calls' lists with tables, n_tables, stack_table behind n_stacks)
        L.dct3d_encode_eg_frames_vq_dev.argtypes = [vp, vp, i32, i32, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp]
        L.dct3d_encode_eg_frames_vq.argtypes = [vp, vp, i32, i32, i32, i32, vp, i32, vp, vp, vp, vp]
        L.dct3d_decode_eg_frames_vq_dev.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp, i32, vp, vp, vp]
        L.dct3d_decode_eg_frames_vq.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp, i32, vp, vp, vp]
        # (the _vq lists: table_map [n_stacks][channels] in the place of stack_table)
        L.dct3d_encode_eg_frames_vqc_dev.argtypes = L.dct3d_encode_eg_frames_vq_dev.argtypes
        L.dct3d_encode_eg_frames_vqc.argtypes = L.dct3d_encode_eg_frames_vq.argtypes
        L.dct3d_decode_eg_frames_vqc_dev.argtypes = L.dct3d_decode_eg_frames_vq_dev.argtypes
        L.dct3d_decode_eg_frames_vqc.argtypes = L.dct3d_decode_eg_frames_vq.argtypes
        L.dct3d_ctx_set_chroma.argtypes = [vp, i32]
        L.dct3d_ctx_get_chroma.argtypes = [vp, C.POINTER(i32)]
        L.dct3d_chroma_size.argtypes = [i32, i32, C.POINTER(i32), C.POINTER(i32)]
        L.dct3d_distortion_rgb_frames_dev.argtypes = [vp, vp, i32, i32, i32, vp, i32, vp, i32, vp, vp, vp, vp]
        L.dct3d_distortion_rgb_frames.argtypes = [vp, vp, i32, i32, i32, vp, i32, vp, i32, vp, vp, vp]
        L.dct3d_ssim_frames_dev.argtypes = [vp, vp, i32, i32, i32, i32, vp, i32, vp, vp, vp, vp]
        L.dct3d_ssim_frames.argtypes = [vp, vp, i32, i32, i32, i32, vp, i32, vp, vp, vp]
        L.dct3d_ssim_windows.argtypes = [i32, i32, C.POINTER(i32), C.POINTER(i32)]
        L.dct3d_ssim_rgb_frames_dev.argtypes = [vp, vp, i32, i32, i32, vp, i32, vp, i32, vp, vp, vp, vp, vp]
        L.dct3d_ssim_rgb_frames.argtypes = [vp, vp, i32, i32, i32, vp, i32, vp, i32, vp, vp, vp, vp]
        _lib = L
    return _lib


_diag = None


def diag_lib() -> C.CDLL:
    """Load libdct3d_diag.so (bench / test support: synthetic frames, memory-only twins, probes)."""
    global _diag
    if _diag is None:
        lib()  # the product library first (the diag library links against it)
        if not os.path.exists(DIAG_LIB_PATH):
            raise ImportError(f"{DIAG_LIB_PATH} is missing: build it with `make`")
        D = C.CDLL(DIAG_LIB_PATH)
        vp, i32, sz, u64, i64 = C.c_void_p, C.c_int, C.c_size_t, C.c_uint64, C.c_int64
        D.dct3d_fill_synthetic_dev.argtypes = [vp, vp, i32, i32, i32, u64, i64, i32]
        D.dct3d_bandwidth_probe_dev.argtypes = [vp, vp, vp, sz, i32]
        D.dct3d_encode_memonly_dev.argtypes = [vp, vp, i32, i32, i32, vp]
        D.dct3d_encode_diag_dev.argtypes = [vp, vp, i32, i32, i32, vp, i32]
        D.dct3d_encode_strip_dev.argtypes = [vp, vp, i32, i32, i32, vp, i32, i32]
        D.dct3d_encode_trace_dev.argtypes = [vp, vp, i32, i32, i32, vp, i32, vp]
        D.dct3d_decode_diag_dev.argtypes = [vp, vp, i32, i32, i32, vp, i32]
        _diag = D
    return _diag


def strerror(code: int) -> str:
    try:
        return lib().dct3d_strerror(code).decode()
    except Exception:
        return "error"


def _check(rc: int, what: str) -> None:
    if rc != DCT3D_OK:
        raise Dct3dError(rc, what)


def _ptr(a: np.ndarray) -> int:
    if not a.flags["C_CONTIGUOUS"]:
        raise ValueError("array must be C-contiguous")
    return a.ctypes.data


def _tptr(t) -> int:
    """device pointer of a torch tensor (or an int address)."""
    if isinstance(t, int):
        return t
    if not t.is_contiguous():
        raise ValueError("tensor must be contiguous")
    return t.data_ptr()


def _steps_array(steps) -> np.ndarray:
    """A quantiser table as the C-ABI takes it (int32, contiguous); values must be whole numbers."""
    a = np.asarray(steps)
    if a.ndim != 1 or not np.all(a == np.floor(a)):
        raise ValueError("a quantiser table is a 1-D array of integer steps")
    return np.ascontiguousarray(a, np.int32)


def quant_table(quality: int, block_d: int = 8) -> np.ndarray:
    """The scalar family of quantiser tables: step[s] = max(1, quality * s) clipped to 255, s = kx + ky + kz,
    8 + 8 + block_d - 2 entries.  quant_table(5) is the reference codec's quantiser."""
    s = np.arange(8 + 8 + block_d - 2, dtype=np.int64)
    return np.clip(int(quality) * s, 1, 255).astype(np.int32)


def _step_cube(steps, shape) -> np.ndarray:
    """step[kx + ky + kz] over a cube array's last three axes [.., bd, bh, bw], as fp64."""
    st = _steps_array(steps)
    bd, bh, bw = shape[-3:]
    if st.size != bw + bh + bd - 2:
        raise ValueError(f"the table of a {bw}x{bh}x{bd} block has {bw + bh + bd - 2} steps")
    z, y, x = np.ogrid[:bd, :bh, :bw]
    return st[x + y + z].astype(np.float64)


def quantize_ref(dct_cubes: np.ndarray, steps) -> np.ndarray:
    """The definition of the quantiser in numpy (Encoder.java:75-89 with step[x + y + z]): fp64 DCT coefficients
    [.., bd, bh, bw] -> int32 Math.round(c / step): an IEEE double division, then exact half-up rounding
    (floor(x + 0.5) misrounds the double below 0.5; Math.round does not)."""
    d = np.asarray(dct_cubes, np.float64)
    v = d / _step_cube(steps, d.shape)
    f = np.floor(v)
    return (f + (v - f >= 0.5)).astype(np.int32)  # v - f is exact: Math.round's floor(v + 1/2) in exact arithmetic


def dequantize_ref(q_cubes: np.ndarray, steps) -> np.ndarray:
    """Decoder.java:78-96 with step[x + y + z]: int32 [.., bd, bh, bw] -> fp64 (double) q * step (exact)."""
    q = np.asarray(q_cubes)
    return q.astype(np.float64) * _step_cube(steps, q.shape)


def _colour_in(frames) -> np.ndarray:
    a = np.asarray(frames)
    if a.ndim < 1 or a.shape[-1] != 3:
        raise ValueError("a colour array's last axis holds the 3 samples of a pixel")
    return a.astype(np.int64)


def ycbcr_to_rgb_unclamped(frames) -> np.ndarray:
    """ycbcr_to_rgb before its clamp to [0, 255]: int64 [.., 3] (the tests' view of what the clamp does)."""
    a = _colour_in(frames)
    y, u, v = a[..., 0], a[..., 1] - 128, a[..., 2] - 128
    return np.stack((y + ((91881 * v + 32768) >> 16), y + ((-22554 * u - 46802 * v + 32768) >> 16),
                     y + ((116130 * u + 32768) >> 16)), axis=-1)


def rgb_to_ycbcr(frames) -> np.ndarray:
    """The definition of DCT3D_COLOUR_YCBCR's forward transform in numpy (dct3d.h): JFIF full-range BT.601 in
    16-bit fixed point, uint8 [.., 3] (R, G, B) -> uint8 [.., 3] (Y, Cb, Cr), int64 inside, >> a floor.  No clamp:
    every numerator lies in [0, 2^24) (tests/test_ycc_ref.py, all 2^24 colours)."""
    a = _colour_in(frames)
    r, g, b = a[..., 0], a[..., 1], a[..., 2]
    out = np.stack(((19595 * r + 38470 * g + 7471 * b + 32768) >> 16,
                    (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16,
                    (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16), axis=-1)
    return out.astype(np.uint8)


def ycbcr_to_rgb(frames) -> np.ndarray:
    """The inverse transform's definition: uint8 [.., 3] (Y, Cb, Cr) -> uint8 [.., 3] (R, G, B), clamped."""
    return np.clip(ycbcr_to_rgb_unclamped(frames), 0, 255).astype(np.uint8)


def chroma_size(w: int, h: int):
    """(cw, ch) of DCT3D_CHROMA_420's chroma planes for w x h frames: ((w + 1) // 2, (h + 1) // 2)."""
    w, h = int(w), int(h)
    if w <= 0 or h <= 0:
        raise ValueError("a frame has at least one pixel")
    return (w + 1) // 2, (h + 1) // 2


def subsample_420(planes) -> np.ndarray:
    """The definition of DCT3D_CHROMA_420's subsampling in numpy (dct3d.h): uint8 planes [.., H, W] -> uint8
    [.., (H + 1) // 2, (W + 1) // 2].  The plane is padded to even width and height by repeating its last column and
    row; then c[j, i] = (p[2j, 2i] + p[2j, 2i+1] + p[2j+1, 2i] + p[2j+1, 2i+1] + 2) >> 2."""
    p = np.asarray(planes)
    if p.ndim < 2 or p.shape[-1] < 1 or p.shape[-2] < 1:
        raise ValueError("planes have shape [.., H, W]")
    p = p.astype(np.int64)
    if p.shape[-1] % 2:
        p = np.concatenate((p, p[..., :, -1:]), axis=-1)
    if p.shape[-2] % 2:
        p = np.concatenate((p, p[..., -1:, :]), axis=-2)
    s = p[..., 0::2, 0::2] + p[..., 0::2, 1::2] + p[..., 1::2, 0::2] + p[..., 1::2, 1::2]
    return ((s + 2) >> 2).astype(np.uint8)


def upsample_420(planes, w: int, h: int) -> np.ndarray:
    """The definition of the upsampling: pixel replication, p[y, x] = c[y >> 1, x >> 1], cropped to w x h; planes
    [.., (h + 1) // 2, (w + 1) // 2] -> [.., h, w], the dtype kept."""
    c = np.asarray(planes)
    if c.ndim < 2 or tuple(c.shape[-2:]) != chroma_size(w, h)[::-1]:
        raise ValueError("the chroma planes of w x h frames have shape [.., (h + 1) // 2, (w + 1) // 2]")
    return np.ascontiguousarray(np.repeat(np.repeat(c, 2, axis=-2), 2, axis=-1)[..., :h, :w])


def rgb_to_ycbcr420(frames):
    """uint8 frames [.., H, W, 3] (R, G, B) -> (Y [.., H, W], Cb, Cr [.., (H + 1) // 2, (W + 1) // 2]): the three
    planes whose grey streams a packed RGB24 stream call writes under DCT3D_CHROMA_420: rgb_to_ycbcr, then
    subsample_420 of its Cb and Cr planes."""
    t = rgb_to_ycbcr(frames)
    if t.ndim < 3:
        raise ValueError("frames have shape [.., H, W, 3]")
    return np.ascontiguousarray(t[..., 0]), subsample_420(t[..., 1]), subsample_420(t[..., 2])


def ycbcr420_to_rgb(y, cb, cr) -> np.ndarray:
    """The inverse: Y [.., H, W] and the chroma planes of rgb_to_ycbcr420 -> uint8 frames [.., H, W, 3]:
    ycbcr_to_rgb of (Y, upsample_420(Cb), upsample_420(Cr))."""
    y = np.asarray(y)
    if y.ndim < 2:
        raise ValueError("Y has shape [.., H, W]")
    h, w = y.shape[-2:]
    return ycbcr_to_rgb(np.stack((y, upsample_420(cb, w, h), upsample_420(cr, w, h)), axis=-1))


RATE_MAX_TABLES = 32


def pick_quality(bits_per_quality: dict, target_bits) -> int:
    """The rate rule of the codec's rate= argument: the smallest quality whose bits are <= target_bits; if none
    fits, the largest quality of the dict.  Nothing is assumed about how the bits vary with the quality."""
    if not bits_per_quality:
        raise ValueError("no qualities to pick from")
    fits = [q for q, b in bits_per_quality.items() if b <= target_bits]
    return int(min(fits)) if fits else int(max(bits_per_quality))


def psnr_db(sse, n_samples) -> float:
    """10 log10(255^2 n_samples / sse) of 8-bit samples; inf for sse == 0."""
    sse = int(sse)
    return float("inf") if sse == 0 else 10.0 * math.log10(255.0 * 255.0 * float(n_samples) / float(sse))


def pick_quality_psnr(sse_per_quality: dict, n_samples, target_db) -> int:
    """The rule of the codec's psnr= argument: the largest quality (the coarsest quantiser) whose PSNR is >=
    target_db; if none reaches it, the smallest quality of the dict.  Nothing is assumed about how the error
    varies with the quality."""
    if not sse_per_quality:
        raise ValueError("no qualities to pick from")
    ok = [q for q, e in sse_per_quality.items() if psnr_db(e, n_samples) >= target_db]
    return int(max(ok)) if ok else int(min(sse_per_quality))


def ssim_windows(w: int, h: int) -> tuple:
    """(nwx, nwy): the SSIM probe's windows of a w x h plane (dct3d_ssim_windows): 8 x 8 windows at a stride of 4
    over the 4 x 4 block grid, nwx = max(ceil(w / 4) - 1, 1)."""
    nwx, nwy = C.c_int(), C.c_int()
    _check(lib().dct3d_ssim_windows(int(w), int(h), C.byref(nwx), C.byref(nwy)), "dct3d_ssim_windows")
    return nwx.value, nwy.value


def ssim_windows_ref(x, y, _parts: bool = False) -> np.ndarray:
    """The SSIM probe's definition (include/dct3d.h) in numpy: uint8 planes x (the source) and y (the decoded
    frames) [.., H, W] -> int64 [.., nwy, nwx], v = floor(s 2^24) of every window.  Blocks: the 4 x 4 grid's integer
    moments n, Sx, Sy, Sxx, Syy, Sxy over the samples inside the plane.  Window (i, j): the sums over blocks
    i .. min(i + 1, nbx - 1) by j .. min(j + 1, nby - 1).  In int64
        A = 20000 Sx Sy + 65025 n^2                  B = 20000 (n Sxy - Sx Sy) + 585225 n^2
        C = 10000 (Sx^2 + Sy^2) + 65025 n^2          D = 10000 (n Sxx - Sx^2 + n Syy - Sy^2) + 585225 n^2
    and in fp64 s = fl(fl(A B) / fl(C D)): two multiplications and one division of exactly converted integers.
    (_parts: the tuple (v, A, B, C, D) instead, for the tests of the bounds.)"""
    x, y = np.asarray(x), np.asarray(y)
    if x.dtype != np.uint8 or y.dtype != np.uint8 or x.shape != y.shape or x.ndim < 2:
        raise ValueError("x and y are uint8 planes [.., H, W] of one shape")
    h, w = x.shape[-2:]
    if h < 1 or w < 1:
        raise ValueError("empty planes")
    nbx, nby = (w + 3) // 4, (h + 3) // 4
    nwx, nwy = max(nbx - 1, 1), max(nby - 1, 1)
    lead = x.shape[:-2]

    def blocks(a):  # the 4 x 4 blocks' sums of a [.., H, W] (zero outside the plane)
        p = np.zeros(lead + (4 * nby, 4 * nbx), np.int64)
        p[..., :h, :w] = a
        return p.reshape(lead + (nby, 4, nbx, 4)).sum(axis=(-3, -1))

    def windows(b):  # blocks -> windows: the 1, 2 or 4 blocks of each
        r = b[..., :nwy, :nwx].copy()
        if nbx > 1:
            r += b[..., :nwy, 1:nwx + 1]
        if nby > 1:
            r += b[..., 1:nwy + 1, :nwx]
        if nbx > 1 and nby > 1:
            r += b[..., 1:nwy + 1, 1:nwx + 1]
        return r

    xi, yi = x.astype(np.int64), y.astype(np.int64)
    n = windows(blocks(np.ones(x.shape, np.int64)))
    Sx, Sy = windows(blocks(xi)), windows(blocks(yi))
    Sxx, Syy, Sxy = windows(blocks(xi * xi)), windows(blocks(yi * yi)), windows(blocks(xi * yi))
    n2 = n * n
    A = 20000 * Sx * Sy + 65025 * n2
    B = 20000 * (n * Sxy - Sx * Sy) + 585225 * n2
    Cc = 10000 * (Sx * Sx + Sy * Sy) + 65025 * n2
    D = 10000 * (n * Sxx - Sx * Sx + n * Syy - Sy * Sy) + 585225 * n2
    s = (A.astype(np.float64) * B.astype(np.float64)) / (Cc.astype(np.float64) * D.astype(np.float64))
    v = np.floor(s * 16777216.0).astype(np.int64)
    return (v, A, B, Cc, D) if _parts else v


def ssim_mean(total, n_windows) -> float:
    """The mean SSIM of n_windows windows whose v sum to total (ssim_frames' numbers, summed as needed):
    total / (2^24 n_windows)."""
    if int(n_windows) < 1:
        raise ValueError("n_windows must be >= 1")
    return float(int(total)) / (16777216.0 * float(int(n_windows)))


def pick_quality_ssim(ssim_per_quality: dict, n_windows, target) -> int:
    """The rule of the codec's ssim= argument: the largest quality (the coarsest quantiser) whose mean SSIM is >=
    target; if none reaches it, the smallest quality of the dict.  Nothing is assumed about how the SSIM varies with
    the quality."""
    if not ssim_per_quality:
        raise ValueError("no qualities to pick from")
    ok = [q for q, t in ssim_per_quality.items() if ssim_mean(t, n_windows) >= target]
    return int(max(ok)) if ok else int(min(ssim_per_quality))


def pick_stack_qualities_ssim(ssim, qualities, n_windows_per_stack, target) -> list:
    """pick_quality_ssim per stack: ssim [T, n_stacks, channels] as ssim_frames returns it for the tables of
    `qualities`; stack s gets pick_quality_ssim of its sums added over the channels, over n_windows_per_stack windows
    (all channels' windows of one stack)."""
    ssim = np.asarray(ssim)
    qualities = [int(q) for q in qualities]
    if ssim.ndim != 3 or ssim.shape[0] != len(qualities):
        raise ValueError("ssim must be [len(qualities), n_stacks, channels]")
    return [pick_quality_ssim({q: int(ssim[t, s, :].astype(object).sum()) for t, q in enumerate(qualities)},
                              n_windows_per_stack, target) for s in range(ssim.shape[1])]


def pick_stack_qualities(bits, qualities, target_bits_per_stack) -> list:
    """pick_quality per stack: bits [T, n_stacks, channels] as rate_frames returns them for the tables of
    `qualities` (T of them); stack s gets pick_quality of its bits summed over the channels against
    target_bits_per_stack.  One quality per stack, in stack order; no other rule, nothing assumed monotone."""
    bits = np.asarray(bits)
    qualities = [int(q) for q in qualities]
    if bits.ndim != 3 or bits.shape[0] != len(qualities):
        raise ValueError("bits must be [len(qualities), n_stacks, channels]")
    return [pick_quality({q: int(bits[t, s, :].astype(object).sum()) for t, q in enumerate(qualities)}, target_bits_per_stack)
            for s in range(bits.shape[1])]


def pick_stack_channel_qualities(bits, qualities, target_bits_per_stack, chroma_rungs=0) -> list:
    """One (q0, q1, q2) per stack for the per-(stack, channel) calls (encode_eg_frames_vqc): bits [T, n_stacks, 3]
    as rate_frames returns them for the tables of `qualities` (T of them, in that order).  Candidate i codes
    channel 0 under qualities[i] and channels 1 and 2 under qualities[j], j = min(i + chroma_rungs, T - 1), and
    costs bits[i, s, 0] + bits[j, s, 1] + bits[j, s, 2]; stack s gets pick_quality's choice on these costs (the
    smallest quality that fits target_bits_per_stack, else the largest quality).  Nothing assumed monotone."""
    bits = np.asarray(bits)
    qualities = [int(q) for q in qualities]
    T = len(qualities)
    if bits.ndim != 3 or bits.shape[0] != T or bits.shape[2] != 3:
        raise ValueError("bits must be [len(qualities), n_stacks, 3]")
    if int(chroma_rungs) != chroma_rungs or chroma_rungs < 0:
        raise ValueError("chroma_rungs must be an integer >= 0")
    j = [min(i + int(chroma_rungs), T - 1) for i in range(T)]
    index = {q: i for i, q in enumerate(qualities)}
    res = []
    for s in range(bits.shape[1]):
        q = pick_quality({qualities[i]: int(bits[i, s, 0]) + int(bits[j[i], s, 1]) + int(bits[j[i], s, 2]) for i in range(T)},
                         target_bits_per_stack)
        res.append((q, qualities[j[index[q]]], qualities[j[index[q]]]))
    return res


def pick_stack_qualities_psnr(sse, qualities, n_samples_per_stack, target_db) -> list:
    """pick_quality_psnr per stack: sse [T, n_stacks, channels] as distortion_frames returns it for the tables of
    `qualities`; stack s gets pick_quality_psnr of its squared error summed over the channels, over
    n_samples_per_stack samples (all channels' unpadded samples of one stack)."""
    sse = np.asarray(sse)
    qualities = [int(q) for q in qualities]
    if sse.ndim != 3 or sse.shape[0] != len(qualities):
        raise ValueError("sse must be [len(qualities), n_stacks, channels]")
    return [pick_quality_psnr({q: int(sse[t, s, :].astype(object).sum()) for t, q in enumerate(qualities)},
                              n_samples_per_stack, target_db) for s in range(sse.shape[1])]


def pick_stack_channel_qualities_psnr(sse, qualities, n_samples_per_stack, target_db, chroma_rungs=0) -> list:
    """One (q0, q1, q2) per stack from the RGB-domain distortion probe: sse [T, n_stacks] as distortion_rgb_frames
    returns it for the T candidates (qualities[i], qualities[j], qualities[j]), j = min(i + chroma_rungs, T - 1), in
    that order.  Stack s gets pick_quality_psnr's choice on its errors over n_samples_per_stack samples (the three
    bytes of one stack's unpadded pixels): the largest qualities[i] whose PSNR is >= target_db, else the smallest.
    Mirrors pick_stack_channel_qualities; nothing assumed monotone."""
    sse = np.asarray(sse)
    qualities = [int(q) for q in qualities]
    T = len(qualities)
    if sse.ndim != 2 or sse.shape[0] != T:
        raise ValueError("sse must be [len(qualities), n_stacks]")
    if int(chroma_rungs) != chroma_rungs or chroma_rungs < 0:
        raise ValueError("chroma_rungs must be an integer >= 0")
    j = [min(i + int(chroma_rungs), T - 1) for i in range(T)]
    index = {q: i for i, q in enumerate(qualities)}
    res = []
    for s in range(sse.shape[1]):
        q = pick_quality_psnr({qualities[i]: int(sse[i, s]) for i in range(T)}, n_samples_per_stack, target_db)
        res.append((q, qualities[j[index[q]]], qualities[j[index[q]]]))
    return res


def pick_stack_channel_qualities_ssim(ssim, qualities, n_windows_per_stack, target, chroma_rungs=0) -> list:
    """One (q0, q1, q2) per stack from the RGB and luma SSIM probe: ssim [T, n_stacks, 3] as ssim_rgb_frames returns
    it for the T candidates (qualities[i], qualities[j], qualities[j]), j = min(i + chroma_rungs, T - 1), in that order.
    Stack s gets pick_quality_ssim's choice on its sums added over R, G and B, over n_windows_per_stack windows (the
    three planes' windows of one stack): the largest qualities[i] whose mean SSIM is >= target, else the smallest.
    Mirrors pick_stack_channel_qualities_psnr; nothing assumed monotone."""
    ssim = np.asarray(ssim)
    qualities = [int(q) for q in qualities]
    T = len(qualities)
    if ssim.ndim != 3 or ssim.shape[0] != T or ssim.shape[2] != 3:
        raise ValueError("ssim must be [len(qualities), n_stacks, 3]")
    if int(chroma_rungs) != chroma_rungs or chroma_rungs < 0:
        raise ValueError("chroma_rungs must be an integer >= 0")
    j = [min(i + int(chroma_rungs), T - 1) for i in range(T)]
    index = {q: i for i, q in enumerate(qualities)}
    res = []
    for s in range(ssim.shape[1]):
        q = pick_quality_ssim({qualities[i]: sum(int(v) for v in ssim[i, s, :]) for i in range(T)}, n_windows_per_stack, target)
        res.append((q, qualities[j[index[q]]], qualities[j[index[q]]]))
    return res


def plan_query(block_w: int = 8, block_h: int = 8, block_d: int = 8, steps=None) -> dict:
    """Host-side transform plan (no device): Java fold tables + certification tables, for the quantiser
    table `steps` (None: the reference's)."""
    cs = block_w * block_h * block_d
    info = PlanInfo()
    ng = np.empty(cs, np.int32)
    coef = np.empty(cs * 64, np.float64)
    gof = np.empty(cs * cs, np.uint8)
    K = np.empty(cs, np.float64)
    if steps is None:
        _check(lib().dct3d_plan_query(block_w, block_h, block_d, C.byref(info), _ptr(ng), _ptr(coef), _ptr(gof), _ptr(K)),
               "dct3d_plan_query")
    else:
        st = _steps_array(steps)
        _check(lib().dct3d_plan_query_quant(block_w, block_h, block_d, _ptr(st), st.size, C.byref(info), _ptr(ng),
                                            _ptr(coef), _ptr(gof), _ptr(K)), "dct3d_plan_query_quant")
    return {"cube_size": info.cube_size, "n_mults": info.n_mults, "treeified": bool(info.treeified),
            "coef_dc": info.coef_dc, "dec_G": info.dec_G, "dec_E": info.dec_E, "dec_l1_max": info.dec_l1_max,
            "enc_rstep": np.array(info.enc_rstep[:]), "enc_G": np.array(info.enc_G[:]),
            "enc_E": np.array(info.enc_E[:]), "enc_thr64": np.array(info.enc_thr64[:]), "ngroups": ng, "coef": coef.reshape(cs, 64),
            "group_of": gof.reshape(cs, cs), "enc_K": K}


def diagonal_order(block_w: int = 8, block_h: int = 8, block_d: int = 8) -> np.ndarray:
    """Diagonal-slice order used by the device Exp-Golomb stage: cube index x + 8y + 64z per stream
    position (CubeUtils.c:5-46)."""
    out = np.empty(block_w * block_h * block_d, np.uint16)
    _check(lib().dct3d_diagonal_order(block_w, block_h, block_d, _ptr(out)), "dct3d_diagonal_order")
    return out


def padded_size(width: int, height: int) -> tuple[int, int]:
    """(Wp, Hp): width and height rounded up to multiples of 8, the size of the padded raster that
    encode_frames / decode_frames are defined on."""
    return (width + 7) // 8 * 8, (height + 7) // 8 * 8


def pad_frames(frames: np.ndarray) -> np.ndarray:
    """The padded raster of frames [F, H, W] (grey) or [F, H, W, 3] (packed RGB24): each frame's last column
    and last row repeated up to padded_size (per channel).  This is the definition of what encode_frames
    encodes -- the calls themselves never build it."""
    frames = np.asarray(frames)
    if frames.ndim not in (3, 4) or (frames.ndim == 4 and frames.shape[3] != 3):
        raise ValueError("frames must have shape [F, H, W] or [F, H, W, 3]")
    H, W = frames.shape[1:3]
    Wp, Hp = padded_size(W, H)
    return np.pad(frames, ((0, 0), (0, Hp - H), (0, Wp - W)) + ((0, 0),) * (frames.ndim - 3), mode="edge")


def eg_stream_bytes(total_bits: int) -> int:
    """Bytes holding a stream of total_bits bits (the last one partial)."""
    return (total_bits + 7) // 8


class Context:
    """dct3d_ctx: one per device (the MI355X equivalent of the reference's per-call OpenCL setup,
    encoder.c:147-197).  Block dims are codec.h's DCT_BLOCK_WIDTH/HEIGHT/DEPTH (8x8x8 or 8x8x4)."""

    def __init__(self, device: int = 0, block_w: int = 8, block_h: int = 8, block_d: int = 8):
        h = C.c_void_p()
        _check(lib().dct3d_ctx_create(device, block_w, block_h, block_d, C.byref(h)), "dct3d_ctx_create")
        self._h = h
        self.device, self.bw, self.bh, self.bd = device, block_w, block_h, block_d
        self.cube_size = block_w * block_h * block_d

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().dct3d_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- configuration ----
    def set_stream(self, hip_stream: Optional[int]) -> None:
        """Run on an external hipStream_t.  None or 0 (e.g. torch's default stream, whose handle is 0)
        selects the context's own stream -- use a non-default stream to share one with a framework."""
        _check(lib().dct3d_ctx_set_stream(self._h, hip_stream or None), "dct3d_ctx_set_stream")

    def set_option(self, option: int, value: float) -> None:
        """Test / diagnostic option (DCT3D_OPT_*): changes how later calls reach their (identical)
        results, e.g. to drive a rare path.  0 restores the default."""
        _check(lib().dct3d_ctx_set_option(self._h, option, float(value)), "dct3d_ctx_set_option")

    def set_chroma(self, mode: int) -> None:
        """DCT3D_CHROMA_444 (the default) or DCT3D_CHROMA_420: with the colour transform on, the packed RGB24 stream
        calls and the rate probe code Cb and Cr at a quarter of the samples (rgb_to_ycbcr420)."""
        _check(lib().dct3d_ctx_set_chroma(self._h, int(mode)), "dct3d_ctx_set_chroma")

    def chroma(self) -> int:
        """The context's chroma mode."""
        m = C.c_int(0)
        _check(lib().dct3d_ctx_get_chroma(self._h, C.byref(m)), "dct3d_ctx_get_chroma")
        return m.value

    def set_quant(self, steps) -> None:
        """The context's quantiser table: one integer step in [1, 255] per s = kx + ky + kz (bw + bh + bd - 2
        entries; quant_table()), or None for the reference table.  Every later raster call encodes and decodes
        with it.  Waits for the context's stream; not to be called while another thread has a call in flight."""
        if steps is None:
            _check(lib().dct3d_ctx_set_quant(self._h, None, 0), "dct3d_ctx_set_quant")
        else:
            st = _steps_array(steps)
            _check(lib().dct3d_ctx_set_quant(self._h, _ptr(st), st.size), "dct3d_ctx_set_quant")

    def quant(self) -> np.ndarray:
        """The context's quantiser table (int32 [bw + bh + bd - 2])."""
        st = np.empty(self.bw + self.bh + self.bd - 2, np.int32)
        _check(lib().dct3d_ctx_get_quant(self._h, _ptr(st), st.size), "dct3d_ctx_get_quant")
        return st

    def set_profiling(self, on: bool) -> None:
        _check(lib().dct3d_ctx_set_profiling(self._h, 1 if on else 0), "dct3d_ctx_set_profiling")

    def synchronize(self) -> None:
        _check(lib().dct3d_synchronize(self._h), "dct3d_synchronize")

    def stats(self) -> dict:
        st = Stats()
        _check(lib().dct3d_get_stats(self._h, C.byref(st)), "dct3d_get_stats")
        return st.as_dict()

    def eg_sync_launches(self) -> tuple:
        """(max per front, sum): the sync launches the last stream decode call's fronts issued, the speculative
        attempt and its rerun together (dct3d_eg_sync_launches); one stream: both are its count."""
        mx, sm = C.c_uint64(), C.c_uint64()
        _check(lib().dct3d_eg_sync_launches(self._h, C.byref(mx), C.byref(sm)), "dct3d_eg_sync_launches")
        return mx.value, sm.value

    def reset_timers(self) -> None:
        _check(lib().dct3d_reset_timers(self._h), "dct3d_reset_timers")

    def n_cubes(self, width: int, height: int, n_stacks: int) -> int:
        return (width // self.bw) * (height // self.bh) * n_stacks

    # ---- host-pointer (synchronous) entry points ----
    def encode_stacks(self, frames: np.ndarray, want_dct: bool = False):
        """u8 frames [n_stacks*bd, H, W] -> quantised int32 cubes [n_cubes, bd, bh, bw]
        (+ fp64 DCT coefficients in the same layout when want_dct)."""
        frames = np.ascontiguousarray(frames, np.uint8)
        F, H, W = frames.shape
        if F % self.bd:
            raise ValueError("frame count must be a multiple of the block depth")
        n = self.n_cubes(W, H, F // self.bd)
        q = np.empty((n, self.bd, self.bh, self.bw), np.int32)
        d = np.empty((n, self.bd, self.bh, self.bw), np.float64) if want_dct else None
        _check(lib().dct3d_encode_stacks(self._h, _ptr(frames), W, H, F // self.bd, _ptr(q),
                                         _ptr(d) if want_dct else None), "dct3d_encode_stacks")
        return (q, d) if want_dct else q

    def decode_stacks(self, q: np.ndarray, width: int, height: int, n_stacks: int) -> np.ndarray:
        q = np.ascontiguousarray(q, np.int32)
        out = np.empty((n_stacks * self.bd, height, width), np.uint8)
        _check(lib().dct3d_decode_stacks(self._h, _ptr(q), width, height, n_stacks, _ptr(out)),
               "dct3d_decode_stacks")
        return out

    # packed RGB24 (uint8 [frame][y][x][3]); q is laid out [stack][channel][cube]: block (s, ch) is what
    # encode_stacks gives for stack s of channel ch's plane (include/dct3d.h)
    def encode_stacks_rgb(self, frames: np.ndarray) -> np.ndarray:
        """packed RGB24 frames [n_stacks*bd, H, W, 3] -> quantised int32 cubes [3 * n_cubes, bd, bh, bw],
        equal to encode_stacks of the planar-stacked raster (per stack: its R, then G, then B frames)."""
        frames = np.ascontiguousarray(frames, np.uint8)
        if frames.ndim != 4 or frames.shape[3] != 3:
            raise ValueError("packed RGB24 frames must have shape [F, H, W, 3]")
        F, H, W, _ = frames.shape
        if F % self.bd:
            raise ValueError("frame count must be a multiple of the block depth")
        n = self.n_cubes(W, H, F // self.bd)
        q = np.empty((3 * n, self.bd, self.bh, self.bw), np.int32)
        _check(lib().dct3d_encode_stacks_rgb(self._h, _ptr(frames), W, H, F // self.bd, _ptr(q)),
               "dct3d_encode_stacks_rgb")
        return q

    def decode_stacks_rgb(self, q: np.ndarray, width: int, height: int, n_stacks: int) -> np.ndarray:
        """the inverse of encode_stacks_rgb: packed RGB24 frames [n_stacks*bd, H, W, 3]"""
        q = np.ascontiguousarray(q, np.int32)
        if q.size != 3 * self.n_cubes(width, height, n_stacks) * self.cube_size:
            raise ValueError("q must hold 3 * n_cubes cubes")
        out = np.empty((n_stacks * self.bd, height, width, 3), np.uint8)
        _check(lib().dct3d_decode_stacks_rgb(self._h, _ptr(q), width, height, n_stacks, _ptr(out)),
               "dct3d_decode_stacks_rgb")
        return out

    # frames of any size (include/dct3d.h): the results are those of encode_stacks[_rgb] / decode_stacks[_rgb]
    # on pad_frames(frames), cropped on the way back; the padding and the crop happen inside the kernels
    def encode_frames(self, frames: np.ndarray) -> np.ndarray:
        """u8 frames [n_stacks*bd, H, W] (grey) or [n_stacks*bd, H, W, 3] (packed RGB24), any H, W >= 1 ->
        quantised int32 cubes [channels * n_cubes, bd, bh, bw] of the edge-padded raster (pad_frames)."""
        frames = np.ascontiguousarray(frames, np.uint8)
        if frames.ndim not in (3, 4) or (frames.ndim == 4 and frames.shape[3] != 3):
            raise ValueError("frames must have shape [F, H, W] or [F, H, W, 3]")
        channels = 1 if frames.ndim == 3 else 3
        F, H, W = frames.shape[:3]
        if F % self.bd:
            raise ValueError("frame count must be a multiple of the block depth")
        Wp, Hp = padded_size(W, H)
        q = np.empty((channels * self.n_cubes(Wp, Hp, F // self.bd), self.bd, self.bh, self.bw), np.int32)
        _check(lib().dct3d_encode_frames(self._h, _ptr(frames), W, H, channels, F // self.bd, _ptr(q)),
               "dct3d_encode_frames")
        return q

    def decode_frames(self, q: np.ndarray, width: int, height: int, n_stacks: int, channels: int = 1) -> np.ndarray:
        """the inverse of encode_frames: u8 frames [n_stacks*bd, height, width] (channels = 1) or
        [n_stacks*bd, height, width, 3] (channels = 3), the top-left part of the padded raster's decode"""
        q = np.ascontiguousarray(q, np.int32)
        if channels not in (1, 3):
            raise Dct3dError(DCT3D_EINVAL, "dct3d_decode_frames")
        Wp, Hp = padded_size(width, height)
        if q.size != channels * self.n_cubes(Wp, Hp, n_stacks) * self.cube_size:
            raise ValueError("q must hold channels * n_cubes cubes of the padded raster")
        out = np.empty((n_stacks * self.bd, height, width) + ((3,) if channels == 3 else ()), np.uint8)
        _check(lib().dct3d_decode_frames(self._h, _ptr(q), width, height, channels, n_stacks, _ptr(out)),
               "dct3d_decode_frames")
        return out

    def forward_f32(self, cubes: np.ndarray) -> np.ndarray:
        cubes = np.ascontiguousarray(cubes, np.float32)
        n = cubes.size // self.cube_size
        out = np.empty_like(cubes)
        _check(lib().dct3d_forward_f32(self._h, _ptr(cubes), n, _ptr(out)), "dct3d_forward_f32")
        return out

    def inverse_f32(self, coeffs: np.ndarray) -> np.ndarray:
        coeffs = np.ascontiguousarray(coeffs, np.float32)
        n = coeffs.size // self.cube_size
        out = np.empty_like(coeffs)
        _check(lib().dct3d_inverse_f32(self._h, _ptr(coeffs), n, _ptr(out)), "dct3d_inverse_f32")
        return out

    # ---- device-pointer (asynchronous, ctx stream) entry points ----
    def encode_stacks_dev(self, d_frames, width: int, height: int, n_stacks: int, d_q, d_dct=None) -> None:
        _check(lib().dct3d_encode_stacks_dev(self._h, _tptr(d_frames), width, height, n_stacks, _tptr(d_q),
                                             _tptr(d_dct) if d_dct is not None else None),
               "dct3d_encode_stacks_dev")

    def decode_stacks_dev(self, d_q, width: int, height: int, n_stacks: int, d_frames) -> None:
        _check(lib().dct3d_decode_stacks_dev(self._h, _tptr(d_q), width, height, n_stacks, _tptr(d_frames)),
               "dct3d_decode_stacks_dev")

    def encode_stacks_rgb_dev(self, d_frames, width: int, height: int, n_stacks: int, d_q) -> None:
        _check(lib().dct3d_encode_stacks_rgb_dev(self._h, _tptr(d_frames), width, height, n_stacks, _tptr(d_q)),
               "dct3d_encode_stacks_rgb_dev")

    def decode_stacks_rgb_dev(self, d_q, width: int, height: int, n_stacks: int, d_frames) -> None:
        _check(lib().dct3d_decode_stacks_rgb_dev(self._h, _tptr(d_q), width, height, n_stacks, _tptr(d_frames)),
               "dct3d_decode_stacks_rgb_dev")

    def encode_frames_dev(self, d_frames, width: int, height: int, channels: int, n_stacks: int, d_q) -> None:
        _check(lib().dct3d_encode_frames_dev(self._h, _tptr(d_frames), width, height, channels, n_stacks, _tptr(d_q)),
               "dct3d_encode_frames_dev")

    def decode_frames_dev(self, d_q, width: int, height: int, channels: int, n_stacks: int, d_frames) -> None:
        _check(lib().dct3d_decode_frames_dev(self._h, _tptr(d_q), width, height, channels, n_stacks, _tptr(d_frames)),
               "dct3d_decode_frames_dev")

    def forward_f32_dev(self, d_in, n_cubes: int, d_out) -> None:
        _check(lib().dct3d_forward_f32_dev(self._h, _tptr(d_in), n_cubes, _tptr(d_out)), "dct3d_forward_f32_dev")

    def inverse_f32_dev(self, d_in, n_cubes: int, d_out) -> None:
        _check(lib().dct3d_inverse_f32_dev(self._h, _tptr(d_in), n_cubes, _tptr(d_out)), "dct3d_inverse_f32_dev")

    def bandwidth_probe_dev(self, d_in, d_out, n_px: int, mode: int = 0) -> None:
        _check(diag_lib().dct3d_bandwidth_probe_dev(self._h, _tptr(d_in) if d_in is not None else None,
                                               _tptr(d_out) if d_out is not None else None, n_px, mode),
               "dct3d_bandwidth_probe_dev")

    def encode_memonly_dev(self, d_frames, width: int, height: int, n_stacks: int, d_q) -> None:
        """Diagnostic: the encode's memory traffic without its compute (d_q is NOT a DCT)."""
        _check(diag_lib().dct3d_encode_memonly_dev(self._h, _tptr(d_frames), width, height, n_stacks, _tptr(d_q)),
               "dct3d_encode_memonly_dev")

    def encode_strip_dev(self, d_frames, width: int, height: int, n_stacks: int, d_q, mode: int, strip_w: int) -> None:
        """diagnostic traversal sweep (dct3d_encode_strip_dev): mode 1 memory only, mode 0 the full encode"""
        _check(diag_lib().dct3d_encode_strip_dev(self._h, _tptr(d_frames), width, height, n_stacks, _tptr(d_q), mode,
                                                 strip_w), "dct3d_encode_strip_dev")

    def encode_diag_dev(self, d_frames, width: int, height: int, n_stacks: int, d_q, mode: int) -> None:
        """Diagnostic: the encode's memory part (mode 1) or, 8x8x8, its compute part (mode 2) alone."""
        _check(diag_lib().dct3d_encode_diag_dev(self._h, _tptr(d_frames), width, height, n_stacks, _tptr(d_q), mode),
               "dct3d_encode_diag_dev")

    def encode_trace_dev(self, d_frames, width: int, height: int, n_stacks: int, d_q, d_trace) -> None:
        """Diagnostic: the product encode (8x8x8) with a per-wave timeline in d_trace (uint64, 4 per wave:
        start, transform done, stores issued -- 100 MHz clock -- and XCC_ID << 32 | HW_ID)."""
        _check(diag_lib().dct3d_encode_trace_dev(self._h, _tptr(d_frames), width, height, n_stacks, _tptr(d_q), 3,
                                                 _tptr(d_trace)), "dct3d_encode_trace_dev")

    def decode_diag_dev(self, d_q, width: int, height: int, n_stacks: int, d_frames, mode: int) -> None:
        """Diagnostic: the decode's memory part (mode 1) or compute part (mode 2) alone."""
        _check(diag_lib().dct3d_decode_diag_dev(self._h, _tptr(d_q), width, height, n_stacks, _tptr(d_frames), mode),
               "dct3d_decode_diag_dev")

    # ---- Exp-Golomb stage ----
    def eg_encode_dev(self, d_q, n_cubes: int, d_out, out_cap: int, carry_byte: int = 0, carry_bits: int = 0) -> int:
        """Device Exp-Golomb stream of n_cubes int32 cubes into d_out (4-byte aligned words); returns the
        total bits (carry included) as soon as they are known: the last words of d_out complete on the context
        stream (synchronize() or stream order), and d_q / d_out must stay valid until then.  Raises
        Dct3dError(DCT3D_ENOSPC) when out_cap is too small."""
        tb = C.c_uint64(0)
        _check(lib().dct3d_eg_encode_dev(self._h, _tptr(d_q), n_cubes, carry_byte, carry_bits, _tptr(d_out), out_cap,
                                         C.byref(tb)), "dct3d_eg_encode_dev")
        return tb.value

    def encode_eg_dev(self, d_frames, width: int, height: int, n_stacks: int, d_out, out_cap: int,
                      carry_byte: int = 0, carry_bits: int = 0) -> int:
        """Fused device path: u8 frames (device) -> Exp-Golomb stream words in d_out, no int32
        intermediate; returns the total bits (carry included) as soon as they are known: the last words of
        d_out complete on the context stream (synchronize() or stream order), and d_frames / d_out must stay
        valid until then.  Dct3dError(DCT3D_ENOSPC) if out_cap is too small."""
        tb = C.c_uint64(0)
        _check(lib().dct3d_encode_eg_dev(self._h, _tptr(d_frames), width, height, n_stacks, carry_byte, carry_bits,
                                         _tptr(d_out), out_cap, C.byref(tb)), "dct3d_encode_eg_dev")
        return tb.value

    def encode_eg(self, frames: np.ndarray, carry_byte: int = 0, carry_bits: int = 0) -> tuple[bytes, int]:
        """u8 frames [n_stacks*bd, H, W] -> (Exp-Golomb stream bytes, total bits), computed on the device
        (DCT + quantisation + diagonal order + Exp-Golomb); only the stream crosses PCIe."""
        frames = np.ascontiguousarray(frames, np.uint8)
        F, H, W = frames.shape
        if F % self.bd:
            raise ValueError("frame count must be a multiple of the block depth")
        tb = C.c_uint64(0)
        _check(lib().dct3d_encode_eg(self._h, _ptr(frames), W, H, F // self.bd, carry_byte, carry_bits, C.byref(tb)),
               "dct3d_encode_eg")
        out = np.empty(eg_stream_bytes(tb.value), np.uint8)
        _check(lib().dct3d_eg_fetch(self._h, _ptr(out) if out.size else None, out.size), "dct3d_eg_fetch")
        return out.tobytes(), tb.value

    def eg_decode_dev(self, d_bytes, nbytes: int, start_bit: int, n_cubes: int, d_q) -> int:
        """Device Exp-Golomb stream (4-byte aligned) -> n_cubes cube-major int32 cubes; returns the bit
        after the last value.  Dct3dError(DCT3D_ENODATA) if the stream is too short."""
        eb = C.c_uint64(0)
        _check(lib().dct3d_eg_decode_dev(self._h, _tptr(d_bytes), nbytes, start_bit, n_cubes, _tptr(d_q), C.byref(eb)),
               "dct3d_eg_decode_dev")
        return eb.value

    def decode_eg_dev(self, d_bytes, nbytes: int, start_bit: int, width: int, height: int, n_stacks: int,
                      d_frames) -> int:
        """Fused device path: Exp-Golomb stream (device, 4-byte aligned) -> u8 frames (device), no int32
        intermediate; returns the bit after the last value once the stream's verdict is known -- the frames
        complete asynchronously on the context stream (as decode_stacks_dev; synchronize() or stream order)."""
        eb = C.c_uint64(0)
        _check(lib().dct3d_decode_eg_dev(self._h, _tptr(d_bytes), nbytes, start_bit, width, height, n_stacks,
                                         _tptr(d_frames), C.byref(eb)), "dct3d_decode_eg_dev")
        return eb.value

    def decode_eg(self, stream: bytes, width: int, height: int, n_stacks: int, start_bit: int = 0):
        """Exp-Golomb stream bytes (from bit start_bit, 0..7) -> (u8 frames [n_stacks*bd, H, W], end bit):
        entropy decode + dequantise + IDCT on the device."""
        b = np.frombuffer(stream, np.uint8)
        out = np.empty((n_stacks * self.bd, height, width), np.uint8)
        eb = C.c_uint64(0)
        _check(lib().dct3d_decode_eg(self._h, _ptr(b) if b.size else None, b.size, start_bit, width, height, n_stacks,
                                     _ptr(out), C.byref(eb)), "dct3d_decode_eg")
        return out, eb.value

    # ---- fused stream calls for frames of any size, grey or packed RGB24: one stream per channel ----
    @staticmethod
    def _frames_shape(frames: np.ndarray, bd: int):
        if frames.ndim not in (3, 4) or (frames.ndim == 4 and frames.shape[3] != 3):
            raise ValueError("frames must have shape [F, H, W] or [F, H, W, 3]")
        if frames.shape[0] % bd:
            raise ValueError("frame count must be a multiple of the block depth")
        return 1 if frames.ndim == 3 else 3, frames.shape[0] // bd, frames.shape[1], frames.shape[2]

    def encode_eg_frames(self, frames: np.ndarray, carry=None) -> list:
        """u8 frames [n_stacks*bd, H, W] (grey) or [n_stacks*bd, H, W, 3] (packed RGB24), any H, W >= 1 -> one
        (Exp-Golomb stream bytes, total bits) per channel: the stream of that channel's cubes of
        encode_frames(frames), in stack order.  carry: per channel (carry_byte, carry_bits), default (0, 0)."""
        frames = np.ascontiguousarray(frames, np.uint8)
        channels, n_stacks, H, W = self._frames_shape(frames, self.bd)
        carry = list(carry) if carry is not None else [(0, 0)] * channels
        if len(carry) != channels:
            raise ValueError("one (carry_byte, carry_bits) per channel")
        cb = (C.c_uint8 * channels)(*[b for b, _ in carry])
        cn = (C.c_int * channels)(*[n for _, n in carry])
        tb = (C.c_uint64 * channels)()
        _check(lib().dct3d_encode_eg_frames(self._h, _ptr(frames), W, H, channels, n_stacks, cb, cn, tb),
               "dct3d_encode_eg_frames")
        res = []
        for ch in range(channels):
            out = np.empty(eg_stream_bytes(tb[ch]), np.uint8)
            _check(lib().dct3d_eg_fetch_channel(self._h, ch, _ptr(out) if out.size else None, out.size),
                   "dct3d_eg_fetch_channel")
            res.append((out.tobytes(), int(tb[ch])))
        return res

    def decode_eg_frames(self, streams, width: int, height: int, n_stacks: int, start_bits=None):
        """one Exp-Golomb stream (bytes) per channel, each from bit start_bits[ch] (0..7) -> (u8 frames
        [n_stacks*bd, height, width] for one stream, [n_stacks*bd, height, width, 3] for three; end bits)."""
        channels = len(streams)
        if channels not in (1, 3):
            raise Dct3dError(DCT3D_EINVAL, "dct3d_decode_eg_frames")
        start_bits = list(start_bits) if start_bits is not None else [0] * channels
        bufs = [np.frombuffer(b, np.uint8) for b in streams]
        ptrs = (C.c_void_p * channels)(*[_ptr(b) if b.size else None for b in bufs])
        nb = (C.c_uint64 * channels)(*[b.size for b in bufs])
        sb = (C.c_int * channels)(*start_bits)
        eb = (C.c_uint64 * channels)()
        out = np.empty((n_stacks * self.bd, height, width) + ((3,) if channels == 3 else ()), np.uint8)
        _check(lib().dct3d_decode_eg_frames(self._h, ptrs, nb, sb, width, height, channels, n_stacks, _ptr(out), eb),
               "dct3d_decode_eg_frames")
        return out, [int(e) for e in eb]

    def encode_eg_frames_dev(self, d_frames, width: int, height: int, channels: int, n_stacks: int, d_outs, out_caps,
                             carry=None) -> list:
        """Fused device path: u8 frames (device) -> channel ch's stream words in d_outs[ch] (tensors or
        addresses, 4-byte aligned, out_caps[ch] bytes), no int32 intermediate; returns the total bits per
        channel.  Dct3dError(DCT3D_ENOSPC) if a capacity is too small (its .total_bits holds the totals)."""
        carry = list(carry) if carry is not None else [(0, 0)] * channels
        cb = (C.c_uint8 * channels)(*[b for b, _ in carry])
        cn = (C.c_int * channels)(*[n for _, n in carry])
        outs = (C.c_void_p * channels)(*[_tptr(t) for t in d_outs])
        caps = (C.c_uint64 * channels)(*out_caps)
        tb = (C.c_uint64 * channels)()
        rc = lib().dct3d_encode_eg_frames_dev(self._h, _tptr(d_frames), width, height, channels, n_stacks, cb, cn, outs,
                                              caps, tb)
        if rc != DCT3D_OK:
            e = Dct3dError(rc, "dct3d_encode_eg_frames_dev")
            e.total_bits = [int(t) for t in tb]
            raise e
        return [int(t) for t in tb]

    def decode_eg_frames_dev(self, d_streams, nbytes, start_bits, width: int, height: int, n_stacks: int, d_frames) -> list:
        """Fused device path: one Exp-Golomb stream per channel (tensors or addresses, 4-byte aligned) -> u8
        frames (device), no int32 intermediate; returns the end bit per channel.  On a short or corrupt stream
        the Dct3dError's .end_bits holds the end bits of the streams that were good."""
        channels = len(d_streams)
        ptrs = (C.c_void_p * channels)(*[_tptr(t) for t in d_streams])
        nb = (C.c_uint64 * channels)(*nbytes)
        sb = (C.c_uint64 * channels)(*start_bits)
        eb = (C.c_uint64 * channels)()
        rc = lib().dct3d_decode_eg_frames_dev(self._h, ptrs, nb, sb, width, height, channels, n_stacks, _tptr(d_frames), eb)
        if rc != DCT3D_OK:
            e = Dct3dError(rc, "dct3d_decode_eg_frames_dev")
            e.end_bits = [int(t) for t in eb]
            raise e
        return [int(t) for t in eb]

    # ---- the same four calls with a quantiser table per stack (include/dct3d.h) ----
    # (and, the _vqc names, per (stack, channel): DESIGN 4r.  Each pair shares one body: `what` is the C-ABI call,
    # map_channels None for a map per stack, else the map's second dimension.)
    def _vq_args(self, tables, stack_table, n_stacks: int, what: str, map_channels=None):
        """(int32 [T, n_steps], T, uint8 [n_stacks] or [n_stacks, map_channels]) as the C-ABI takes them; a wrong
        shape is DCT3D_EINVAL"""
        if tables is None or stack_table is None:
            raise Dct3dError(DCT3D_EINVAL, what)
        tb, T = self._rate_tables(tables)
        m = np.asarray(stack_table)
        shape = (n_stacks,) if map_channels is None else (n_stacks, map_channels)
        if m.shape != shape or np.any(m < 0) or np.any(m > 255) or np.any(m != np.floor(m)):
            raise Dct3dError(DCT3D_EINVAL, what)
        return tb, T, np.ascontiguousarray(m, np.uint8)

    def encode_eg_frames_vq(self, frames: np.ndarray, tables, stack_table, carry=None) -> list:
        """encode_eg_frames with stack s of every channel coded under tables[stack_table[s]] (a palette of 1..32
        tables, one uint8 entry per stack).  The context's quantiser is neither used nor changed."""
        return self._encode_eg_frames_vq(frames, tables, stack_table, carry, "dct3d_encode_eg_frames_vq", False)

    def encode_eg_frames_vqc(self, frames: np.ndarray, tables, table_map, carry=None) -> list:
        """encode_eg_frames_vq with a table per (stack, channel): table_map [n_stacks, channels], stack s of channel
        ch coded under tables[table_map[s, ch]] (under the colour transform: of plane ch, Y / Cb / Cr)"""
        return self._encode_eg_frames_vq(frames, tables, table_map, carry, "dct3d_encode_eg_frames_vqc", True)

    def _encode_eg_frames_vq(self, frames, tables, stack_table, carry, what, per_channel) -> list:
        frames = np.ascontiguousarray(frames, np.uint8)
        channels, n_stacks, H, W = self._frames_shape(frames, self.bd)
        tq, T, m = self._vq_args(tables, stack_table, n_stacks, what, channels if per_channel else None)
        carry = list(carry) if carry is not None else [(0, 0)] * channels
        if len(carry) != channels:
            raise ValueError("one (carry_byte, carry_bits) per channel")
        cb = (C.c_uint8 * channels)(*[b for b, _ in carry])
        cn = (C.c_int * channels)(*[n for _, n in carry])
        tb = (C.c_uint64 * channels)()
        _check(getattr(lib(), what)(self._h, _ptr(frames), W, H, channels, n_stacks, _ptr(tq), T, _ptr(m), cb, cn, tb), what)
        res = []
        for ch in range(channels):
            out = np.empty(eg_stream_bytes(tb[ch]), np.uint8)
            _check(lib().dct3d_eg_fetch_channel(self._h, ch, _ptr(out) if out.size else None, out.size),
                   "dct3d_eg_fetch_channel")
            res.append((out.tobytes(), int(tb[ch])))
        return res

    def decode_eg_frames_vq(self, streams, width: int, height: int, n_stacks: int, tables, stack_table, start_bits=None):
        """decode_eg_frames under the same palette and map as encode_eg_frames_vq"""
        return self._decode_eg_frames_vq(streams, width, height, n_stacks, tables, stack_table, start_bits,
                                         "dct3d_decode_eg_frames_vq", False)

    def decode_eg_frames_vqc(self, streams, width: int, height: int, n_stacks: int, tables, table_map, start_bits=None):
        """decode_eg_frames under the same palette and [n_stacks, channels] map as encode_eg_frames_vqc"""
        return self._decode_eg_frames_vq(streams, width, height, n_stacks, tables, table_map, start_bits,
                                         "dct3d_decode_eg_frames_vqc", True)

    def _decode_eg_frames_vq(self, streams, width, height, n_stacks, tables, stack_table, start_bits, what, per_channel):
        channels = len(streams)
        if channels not in (1, 3):
            raise Dct3dError(DCT3D_EINVAL, what)
        tq, T, m = self._vq_args(tables, stack_table, n_stacks, what, channels if per_channel else None)
        start_bits = list(start_bits) if start_bits is not None else [0] * channels
        bufs = [np.frombuffer(b, np.uint8) for b in streams]
        ptrs = (C.c_void_p * channels)(*[_ptr(b) if b.size else None for b in bufs])
        nb = (C.c_uint64 * channels)(*[b.size for b in bufs])
        sb = (C.c_int * channels)(*start_bits)
        eb = (C.c_uint64 * channels)()
        out = np.empty((n_stacks * self.bd, height, width) + ((3,) if channels == 3 else ()), np.uint8)
        rc = getattr(lib(), what)(self._h, ptrs, nb, sb, width, height, channels, n_stacks, _ptr(tq), T, _ptr(m), _ptr(out), eb)
        if rc != DCT3D_OK:
            raise Dct3dError(rc, what)
        return out, [int(e) for e in eb]

    def encode_eg_frames_vq_dev(self, d_frames, width: int, height: int, channels: int, n_stacks: int, tables, stack_table,
                                d_outs, out_caps, carry=None) -> list:
        """encode_eg_frames_dev with a table per stack; errors as there (.total_bits on DCT3D_ENOSPC)"""
        return self._encode_eg_frames_vq_dev(d_frames, width, height, channels, n_stacks, tables, stack_table, d_outs,
                                             out_caps, carry, "dct3d_encode_eg_frames_vq_dev", False)

    def encode_eg_frames_vqc_dev(self, d_frames, width: int, height: int, channels: int, n_stacks: int, tables, table_map,
                                 d_outs, out_caps, carry=None) -> list:
        """encode_eg_frames_vq_dev with table_map [n_stacks, channels]: a table per (stack, channel)"""
        return self._encode_eg_frames_vq_dev(d_frames, width, height, channels, n_stacks, tables, table_map, d_outs,
                                             out_caps, carry, "dct3d_encode_eg_frames_vqc_dev", True)

    def _encode_eg_frames_vq_dev(self, d_frames, width, height, channels, n_stacks, tables, stack_table, d_outs, out_caps,
                                 carry, what, per_channel) -> list:
        tq, T, m = self._vq_args(tables, stack_table, n_stacks, what, channels if per_channel else None)
        carry = list(carry) if carry is not None else [(0, 0)] * channels
        cb = (C.c_uint8 * channels)(*[b for b, _ in carry])
        cn = (C.c_int * channels)(*[n for _, n in carry])
        outs = (C.c_void_p * channels)(*[_tptr(t) for t in d_outs])
        caps = (C.c_uint64 * channels)(*out_caps)
        tb = (C.c_uint64 * channels)()
        rc = getattr(lib(), what)(self._h, _tptr(d_frames), width, height, channels, n_stacks, _ptr(tq), T, _ptr(m), cb, cn,
                                  outs, caps, tb)
        if rc != DCT3D_OK:
            e = Dct3dError(rc, what)
            e.total_bits = [int(t) for t in tb]
            raise e
        return [int(t) for t in tb]

    def decode_eg_frames_vq_dev(self, d_streams, nbytes, start_bits, width: int, height: int, n_stacks: int, tables,
                                stack_table, d_frames) -> list:
        """decode_eg_frames_dev with a table per stack; errors as there (.end_bits of the good streams)"""
        return self._decode_eg_frames_vq_dev(d_streams, nbytes, start_bits, width, height, n_stacks, tables, stack_table,
                                             d_frames, "dct3d_decode_eg_frames_vq_dev", False)

    def decode_eg_frames_vqc_dev(self, d_streams, nbytes, start_bits, width: int, height: int, n_stacks: int, tables,
                                 table_map, d_frames) -> list:
        """decode_eg_frames_vq_dev with table_map [n_stacks, channels]: a table per (stack, channel)"""
        return self._decode_eg_frames_vq_dev(d_streams, nbytes, start_bits, width, height, n_stacks, tables, table_map,
                                             d_frames, "dct3d_decode_eg_frames_vqc_dev", True)

    def _decode_eg_frames_vq_dev(self, d_streams, nbytes, start_bits, width, height, n_stacks, tables, stack_table, d_frames,
                                 what, per_channel) -> list:
        channels = len(d_streams)
        tq, T, m = self._vq_args(tables, stack_table, n_stacks, what, channels if per_channel else None)
        ptrs = (C.c_void_p * channels)(*[_tptr(t) for t in d_streams])
        nb = (C.c_uint64 * channels)(*nbytes)
        sb = (C.c_uint64 * channels)(*start_bits)
        eb = (C.c_uint64 * channels)()
        rc = getattr(lib(), what)(self._h, ptrs, nb, sb, width, height, channels, n_stacks, _ptr(tq), T, _ptr(m),
                                  _tptr(d_frames), eb)
        if rc != DCT3D_OK:
            e = Dct3dError(rc, what)
            e.end_bits = [int(t) for t in eb]
            raise e
        return [int(t) for t in eb]

    # ---- rate probe: the streams' exact sizes under several tables, no stream written ----
    def _rate_tables(self, tables):
        """tables (None | one table | a sequence of tables) -> (int32 [T, n_steps] or None, T)"""
        if tables is None:
            return None, 1
        n = self.bw + self.bh + self.bd - 2
        tb = np.stack([_steps_array(t) for t in ([tables] if np.ndim(tables[0]) == 0 else tables)])
        if tb.shape[1] != n:
            raise Dct3dError(DCT3D_EINVAL, "dct3d_rate_frames")
        return np.ascontiguousarray(tb, np.int32), tb.shape[0]

    def rate_frames(self, frames: np.ndarray, tables=None) -> np.ndarray:
        """u8 frames as encode_eg_frames' -> uint64 [T, n_stacks, channels]: the bits encode_eg_frames appends to
        channel ch's stream for stack s under tables[t] (None: the context's table, T = 1).  Exact; the context's
        quantiser is neither used (tables given) nor changed, and no stream is written."""
        frames = np.ascontiguousarray(frames, np.uint8)
        channels, n_stacks, H, W = self._frames_shape(frames, self.bd)
        tb, T = self._rate_tables(tables)
        bits = np.zeros((T, n_stacks, channels), np.uint64)
        _check(lib().dct3d_rate_frames(self._h, _ptr(frames), W, H, channels, n_stacks, None if tb is None else _ptr(tb), T,
                                       _ptr(bits)), "dct3d_rate_frames")
        return bits

    def rate_frames_dev(self, d_frames, width: int, height: int, channels: int, n_stacks: int, tables=None,
                        d_cube_bits=None) -> np.ndarray:
        """Device path of rate_frames: u8 frames on the device; d_cube_bits (optional; a tensor or an address) receives
        uint16 [T, n_stacks, channels, cubes per stack and channel], the same sum per cube."""
        tb, T = self._rate_tables(tables)
        bits = np.zeros((T, n_stacks, channels), np.uint64)
        _check(lib().dct3d_rate_frames_dev(self._h, _tptr(d_frames), width, height, channels, n_stacks,
                                           None if tb is None else _ptr(tb), T, _ptr(bits),
                                           None if d_cube_bits is None else _tptr(d_cube_bits)), "dct3d_rate_frames_dev")
        return bits

    # ---- distortion probe: the exact squared error of encode + decode under several tables ----
    def distortion_frames(self, frames: np.ndarray, tables=None, want_bits: bool = False):
        """u8 frames as encode_frames' -> uint64 [T, n_stacks, channels]: the sum of (x - y)^2 over the unpadded
        samples of stack s, channel ch, y = decode_frames(encode_frames(x)) under tables[t] (None: the context's
        table, T = 1).  Exact; the context's quantiser is neither used (tables given) nor changed.  want_bits: the
        pair (sse, bits), bits as rate_frames'."""
        frames = np.ascontiguousarray(frames, np.uint8)
        channels, n_stacks, H, W = self._frames_shape(frames, self.bd)
        tb, T = self._rate_tables(tables)
        sse = np.zeros((T, n_stacks, channels), np.uint64)
        bits = np.zeros((T, n_stacks, channels), np.uint64) if want_bits else None
        _check(lib().dct3d_distortion_frames(self._h, _ptr(frames), W, H, channels, n_stacks, None if tb is None else _ptr(tb),
                                             T, _ptr(sse), None if bits is None else _ptr(bits)), "dct3d_distortion_frames")
        return (sse, bits) if want_bits else sse

    def distortion_frames_dev(self, d_frames, width: int, height: int, channels: int, n_stacks: int, tables=None,
                              d_cube_sse=None, want_bits: bool = False):
        """Device path of distortion_frames: u8 frames on the device; d_cube_sse (optional; a tensor or an address)
        receives uint32 [T, n_stacks, channels, cubes per stack and channel], the same sum per cube."""
        tb, T = self._rate_tables(tables)
        sse = np.zeros((T, n_stacks, channels), np.uint64)
        bits = np.zeros((T, n_stacks, channels), np.uint64) if want_bits else None
        _check(lib().dct3d_distortion_frames_dev(self._h, _tptr(d_frames), width, height, channels, n_stacks,
                                                 None if tb is None else _ptr(tb), T, _ptr(sse),
                                                 None if bits is None else _ptr(bits),
                                                 None if d_cube_sse is None else _tptr(d_cube_sse)),
               "dct3d_distortion_frames_dev")
        return (sse, bits) if want_bits else sse

    # ---- SSIM probe: the exact 8 x 8 / stride 4 windowed SSIM of encode + decode under several tables ----
    @staticmethod
    def _ssim_result(ssim, sse, bits):
        if sse is None and bits is None:
            return ssim
        return (ssim,) + (() if sse is None else (sse,)) + (() if bits is None else (bits,))

    def ssim_frames(self, frames: np.ndarray, tables=None, want_sse: bool = False, want_bits: bool = False):
        """u8 frames as encode_frames' -> int64 [T, n_stacks, channels]: the sum of v = floor(s 2^24) over the windows
        of the D frames of stack s, channel ch (ssim_windows_ref states s), y = decode_frames(encode_frames(x)) under
        tables[t] (None: the context's table, T = 1); ssim_mean turns sums into means.  Exact; the context's quantiser
        is neither used (tables given) nor changed.  want_sse / want_bits: the tuple (ssim[, sse][, bits]), sse and
        bits exactly distortion_frames'."""
        frames = np.ascontiguousarray(frames, np.uint8)
        channels, n_stacks, H, W = self._frames_shape(frames, self.bd)
        tb, T = self._rate_tables(tables)
        ssim = np.zeros((T, n_stacks, channels), np.int64)
        sse = np.zeros((T, n_stacks, channels), np.uint64) if want_sse else None
        bits = np.zeros((T, n_stacks, channels), np.uint64) if want_bits else None
        _check(lib().dct3d_ssim_frames(self._h, _ptr(frames), W, H, channels, n_stacks, None if tb is None else _ptr(tb), T,
                                       _ptr(ssim), None if sse is None else _ptr(sse), None if bits is None else _ptr(bits)),
               "dct3d_ssim_frames")
        return self._ssim_result(ssim, sse, bits)

    def ssim_frames_dev(self, d_frames, width: int, height: int, channels: int, n_stacks: int, tables=None,
                        d_window_ssim=None, want_sse: bool = False, want_bits: bool = False):
        """Device path of ssim_frames: u8 frames on the device; d_window_ssim (optional; a tensor or an address)
        receives int32 [T, n_stacks, channels, D, nwy, nwx], the v of every window."""
        tb, T = self._rate_tables(tables)
        ssim = np.zeros((T, n_stacks, channels), np.int64)
        sse = np.zeros((T, n_stacks, channels), np.uint64) if want_sse else None
        bits = np.zeros((T, n_stacks, channels), np.uint64) if want_bits else None
        _check(lib().dct3d_ssim_frames_dev(self._h, _tptr(d_frames), width, height, channels, n_stacks,
                                           None if tb is None else _ptr(tb), T, _ptr(ssim),
                                           None if sse is None else _ptr(sse), None if bits is None else _ptr(bits),
                                           None if d_window_ssim is None else _tptr(d_window_ssim)), "dct3d_ssim_frames_dev")
        return self._ssim_result(ssim, sse, bits)

    # ---- RGB-domain distortion probe: the exact squared error in the RGB pixels under (Y, Cb, Cr) table triples ----
    @staticmethod
    def _rgb_candidates(candidates, T: int, what: str):
        """candidates (None | [n][3] palette indices) -> (uint8 [n, 3] or None, n)"""
        if candidates is None:
            return None, T
        cd = np.ascontiguousarray(candidates, np.int64)
        if cd.ndim != 2 or cd.shape[1] != 3 or cd.shape[0] < 1 or (cd < 0).any() or (cd > 255).any():
            raise Dct3dError(DCT3D_EINVAL, what)
        return np.ascontiguousarray(cd, np.uint8), cd.shape[0]

    def _rgb_result(self, sse, plane_sse, bits, want_planes, want_bits):
        if not want_planes and not want_bits:
            return sse
        return (sse,) + ((plane_sse,) if want_planes else ()) + ((bits,) if want_bits else ())

    def distortion_rgb_frames(self, frames: np.ndarray, tables=None, candidates=None, want_planes: bool = False,
                              want_bits: bool = False):
        """Packed RGB24 frames [n, H, W, 3] -> uint64 [n_cand, n_stacks]: the sum of (x - y)^2 over the unpadded pixels
        of stack s and their three bytes, y = decode_eg_frames_vqc(encode_eg_frames_vqc(x)) with every row of the map
        candidates[c] = (table of Y | R, of Cb | G, of Cr | B), indices into tables, in the context's colour and chroma
        mode.  candidates None: candidate i = (i, i, i).  Exact; the context's quantiser and modes are neither used
        (tables given) nor changed.  want_planes: also the planes' own errors, uint64 [T, n_stacks, 3]; want_bits: also
        the bits, as rate_frames'.  Returns sse, or the tuple (sse[, plane_sse][, bits])."""
        what = "dct3d_distortion_rgb_frames"
        frames = np.ascontiguousarray(frames, np.uint8)
        channels, n_stacks, H, W = self._frames_shape(frames, self.bd)
        if channels != 3:
            raise Dct3dError(DCT3D_EINVAL, what)
        tb, T = self._rate_tables(tables)
        cd, n = self._rgb_candidates(candidates, T, what)
        sse = np.zeros((n, n_stacks), np.uint64)
        plane_sse = np.zeros((T, n_stacks, 3), np.uint64) if want_planes else None
        bits = np.zeros((T, n_stacks, 3), np.uint64) if want_bits else None
        _check(lib().dct3d_distortion_rgb_frames(self._h, _ptr(frames), W, H, n_stacks, None if tb is None else _ptr(tb), T,
                                                 None if cd is None else _ptr(cd), n, _ptr(sse),
                                                 None if plane_sse is None else _ptr(plane_sse),
                                                 None if bits is None else _ptr(bits)), what)
        return self._rgb_result(sse, plane_sse, bits, want_planes, want_bits)

    def distortion_rgb_frames_dev(self, d_frames, width: int, height: int, n_stacks: int, tables=None, candidates=None,
                                  d_cube_sse=None, want_planes: bool = False, want_bits: bool = False):
        """Device path of distortion_rgb_frames: packed RGB24 frames on the device; d_cube_sse (optional; a tensor or an
        address) receives uint32 [n_cand, n_stacks, cubes per stack of the frames' grid], the same sum per cube."""
        what = "dct3d_distortion_rgb_frames_dev"
        tb, T = self._rate_tables(tables)
        cd, n = self._rgb_candidates(candidates, T, what)
        sse = np.zeros((n, n_stacks), np.uint64)
        plane_sse = np.zeros((T, n_stacks, 3), np.uint64) if want_planes else None
        bits = np.zeros((T, n_stacks, 3), np.uint64) if want_bits else None
        _check(lib().dct3d_distortion_rgb_frames_dev(self._h, _tptr(d_frames), width, height, n_stacks,
                                                     None if tb is None else _ptr(tb), T, None if cd is None else _ptr(cd), n,
                                                     _ptr(sse), None if plane_sse is None else _ptr(plane_sse),
                                                     None if bits is None else _ptr(bits),
                                                     None if d_cube_sse is None else _tptr(d_cube_sse)), what)
        return self._rgb_result(sse, plane_sse, bits, want_planes, want_bits)

    # ---- RGB and luma SSIM probe: the SSIM probe's sums on the RGB bytes (and the luma) under table triples ----
    @staticmethod
    def _ssim_rgb_result(ssim, ssim_y, sse, bits):
        rest = tuple(a for a in (ssim_y, sse, bits) if a is not None)
        return (ssim,) + rest if rest else ssim

    def ssim_rgb_frames(self, frames: np.ndarray, tables=None, candidates=None, want_luma: bool = False,
                        want_sse: bool = False, want_bits: bool = False):
        """Packed RGB24 frames [n, H, W, 3] -> int64 [n_cand, n_stacks, 3]: the sum of v (ssim_windows_ref) over the
        windows of the D frames of stack s between plane k (R, G, B) of x and of
        y = decode_eg_frames_vqc(encode_eg_frames_vqc(x)) with every row of the map candidates[c], as
        distortion_rgb_frames takes them, in the context's colour and chroma mode.  want_luma (YCbCr modes): also int64
        [n_cand, n_stacks], the sums between the luma of rgb_to_ycbcr(x) and the decoded Y plane; want_sse: also
        distortion_rgb_frames' sse; want_bits: also its bits.  Returns ssim, or the tuple (ssim[, ssim_y][, sse][, bits])."""
        what = "dct3d_ssim_rgb_frames"
        frames = np.ascontiguousarray(frames, np.uint8)
        channels, n_stacks, H, W = self._frames_shape(frames, self.bd)
        if channels != 3:
            raise Dct3dError(DCT3D_EINVAL, what)
        tb, T = self._rate_tables(tables)
        cd, n = self._rgb_candidates(candidates, T, what)
        ssim = np.zeros((n, n_stacks, 3), np.int64)
        ssim_y = np.zeros((n, n_stacks), np.int64) if want_luma else None
        sse = np.zeros((n, n_stacks), np.uint64) if want_sse else None
        bits = np.zeros((T, n_stacks, 3), np.uint64) if want_bits else None
        _check(lib().dct3d_ssim_rgb_frames(self._h, _ptr(frames), W, H, n_stacks, None if tb is None else _ptr(tb), T,
                                           None if cd is None else _ptr(cd), n, _ptr(ssim),
                                           None if ssim_y is None else _ptr(ssim_y), None if sse is None else _ptr(sse),
                                           None if bits is None else _ptr(bits)), what)
        return self._ssim_rgb_result(ssim, ssim_y, sse, bits)

    def ssim_rgb_frames_dev(self, d_frames, width: int, height: int, n_stacks: int, tables=None, candidates=None,
                            d_window_ssim=None, want_luma: bool = False, want_sse: bool = False, want_bits: bool = False):
        """Device path of ssim_rgb_frames: packed RGB24 frames on the device; d_window_ssim (optional; a tensor or an
        address) receives int32 [n_cand, 3, n_stacks, D, nwy, nwx], the v of every window."""
        what = "dct3d_ssim_rgb_frames_dev"
        tb, T = self._rate_tables(tables)
        cd, n = self._rgb_candidates(candidates, T, what)
        ssim = np.zeros((n, n_stacks, 3), np.int64)
        ssim_y = np.zeros((n, n_stacks), np.int64) if want_luma else None
        sse = np.zeros((n, n_stacks), np.uint64) if want_sse else None
        bits = np.zeros((T, n_stacks, 3), np.uint64) if want_bits else None
        _check(lib().dct3d_ssim_rgb_frames_dev(self._h, _tptr(d_frames), width, height, n_stacks,
                                               None if tb is None else _ptr(tb), T, None if cd is None else _ptr(cd), n,
                                               _ptr(ssim), None if ssim_y is None else _ptr(ssim_y),
                                               None if sse is None else _ptr(sse), None if bits is None else _ptr(bits),
                                               None if d_window_ssim is None else _tptr(d_window_ssim)), what)
        return self._ssim_rgb_result(ssim, ssim_y, sse, bits)

    def fill_synthetic_dev(self, d_frames, width: int, height: int, n_frames: int,
                           seed: int = synthetic.DEFAULT_SEED, frame0: int = 0, kind: str = "ramp") -> None:
        k = {"ramp": 0, "uniform": 1}[kind]
        _check(diag_lib().dct3d_fill_synthetic_dev(self._h, _tptr(d_frames), width, height, n_frames, seed, frame0, k),
               "dct3d_fill_synthetic_dev")
