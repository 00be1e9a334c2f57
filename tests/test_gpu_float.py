"""GPU: the three float kernels against a long-double DCT and against a host emulation of their arithmetic.

cube_f32_kernel<8 | 4, forward | inverse> (dct3d_forward_f32[_dev], dct3d_inverse_f32[_dev]: drop-in (A)) and
fwd64_raster_kernel<8 | 4> (the dct output of dct3d_encode_stacks[_dev]) compute in fp64.  Every case asserts

  (a) equality, bit for bit, with tests/native/emulate_float.cpp: the kernels' pass order over the same butterfly
      source, contraction off on both sides;
  (b) independently of (a): the float32 output inside [f32(ref - eps), f32(ref + eps)], the fp64 output within eps of
      ref, where ref is float_common.dct_ref (long double, from the cosine definition; clipped to [0, 255] for the
      inverse) and eps = 1e-9 max(1, |ref|).

test_float_ref.py checks both references against each other and the cases' preconditions on the CPU.  Device calls
write between two 4 KiB canary bands; the device input of the f32 calls is followed by one cube of NaN, so a read past
n_cubes that reaches an output shows without a fault."""
import numpy as np
import pytest

import float_common as fc
import quant_common as qc

pytestmark = pytest.mark.gpu

FILL = 0xA5  # the canary byte: 0xA5A5A5A5 is the float32 -1.4e-16, not a value any case produces


def _ctx(gpu_ctx8, gpu_ctx4, depth):
    return gpu_ctx8 if depth == 8 else gpu_ctx4


def _host(ctx, x, inverse):
    return (ctx.inverse_f32 if inverse else ctx.forward_f32)(x)


def _dev(ctx, x, inverse):
    """the device entry on x [n, D, 8, 8]: the input followed by a cube of NaN, the output between canary bands"""
    import torch
    n, cs = x.shape[0], x[0].size
    d_in = torch.from_numpy(np.concatenate([x.reshape(n, cs), np.full((1, cs), np.nan, np.float32)])).cuda()
    buf, mid = qc.banded(torch, 4 * n * cs, FILL)
    (ctx.inverse_f32_dev if inverse else ctx.forward_f32_dev)(d_in, n, mid.view(torch.float32))
    ctx.synchronize()
    out, intact = qc.bands_intact(buf, 4 * n * cs, FILL)
    assert intact, "a write outside the output"
    return out.view(np.float32).reshape(x.shape)


def _check(out, c, n=None, window=True):
    """(a) and (b) on the first n cubes of the case; both are evaluated before either is reported"""
    s = slice(0, c.n if n is None else n)
    fails = []
    if not np.array_equal(out, c.emu[s]):
        fails.append(f"(a) {int((out != c.emu[s]).sum())} values differ from the emulation")
    if window:
        lo, hi = fc.f32_window(c.expected()[s])
        bad = ~((lo <= out) & (out <= hi))  # a NaN is outside
        if bad.any():
            fails.append(f"(b) {int(bad.sum())} values outside the float rounding of ref +- 1e-9 max(1, |ref|)")
    assert not fails, "; ".join(fails)


def _cases():
    return [(d, inv, name) for d in (8, 4) for inv in (False, True) for name in fc.case_names(d, inv)]


@pytest.mark.parametrize("depth,inverse,name", _cases(), ids=lambda v: str(v))
def test_cube_f32_host_and_device_entry(gpu_ctx8, gpu_ctx4, depth, inverse, name):
    """Every input through dct3d_*_f32 and dct3d_*_f32_dev.  Forward: every position alone at 255 and at -1000.5 with
    a partial last tile, uniform noise and ramp pixels (24 x 16, 18 / 30 cubes), Gaussian floats (sigma 100: (a)
    only), 277 / 553 random cubes; inverse: mid-grey plus every coefficient alone (unclamped), the oracle's dequantised
    coefficients of the same frames, constant cubes at 0, 255, -3, 300 and 254.5, the coefficients of cubes in
    -20 .. 286; at 8x8x8 also the 64 x 32 x 8 frames of the tests this module replaced."""
    ctx = _ctx(gpu_ctx8, gpu_ctx4, depth)
    c = fc.f32_case(name, depth, inverse)
    for out in (_host(ctx, c.x, inverse), _dev(ctx, c.x, inverse)):
        _check(out, c, window=name != "gauss")


@pytest.mark.parametrize("depth", [8, 4])
def test_inverse_clamp_is_live_at_both_ends(gpu_ctx8, gpu_ctx4, depth):
    """The dequantised coefficients of uniform noise: before the clamp the reference goes below -1 and above 256
    (asserted from dct_ref alone), and the output's extremes are exactly 0.0 and 255.0; the constant cubes come out
    as 0, 255, 0, 255 and the rounding of 254.5"""
    ctx = _ctx(gpu_ctx8, gpu_ctx4, depth)
    c = fc.f32_case("uniform", depth, True)
    assert c.ref.min() < -1.0 and c.ref.max() > 256.0
    for out in (_host(ctx, c.x, True), _dev(ctx, c.x, True)):
        assert out.min() == 0.0 and out.max() == 255.0
        assert np.array_equal(out == 0.0, c.emu == 0.0) and np.array_equal(out == 255.0, c.emu == 255.0)
        assert (out[c.ref < -1e-6] == 0.0).all() and (out[c.ref > 255.0 + 1e-6] == 255.0).all()
    k = fc.f32_case("const", depth, True)
    out = _dev(ctx, k.x, True)
    _check(out, k)
    for g, v in enumerate((0.0, 255.0, 0.0, 255.0)):
        assert (out[g] == v).all()
    assert (out[4] > 254.0).all() and (out[4] < 255.0).all()  # inside the range: not clamped


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("depth", [8, 4])
def test_cube_f32_device_tails(gpu_ctx8, gpu_ctx4, depth, inverse):
    """n = 1 .. 17 T + CPW + 1 cubes through the device entry (T = 16 / 32 cubes per block, CPW = 4 / 8 per wave): 1,
    2, 8, 9, 16 and 18 blocks with whole and partial last waves; a grid that is no multiple of 8 blocks takes
    xcd_tile()'s second arm"""
    ctx = _ctx(gpu_ctx8, gpu_ctx4, depth)
    c = fc.f32_case("pool", depth, inverse)
    for n in fc.tail_counts(depth):
        _check(_dev(ctx, c.x[:n], inverse), c, n)


@pytest.mark.parametrize("depth", [8, 4])
def test_cube_f32_host_entry_reuses_its_buffers(gpu_ctx8, gpu_ctx4, depth):
    """large -> small -> large on one context, both directions: the host entry's work buffers grow once and are
    reused"""
    ctx = _ctx(gpu_ctx8, gpu_ctx4, depth)
    for inverse in (False, True):
        c = fc.f32_case("pool", depth, inverse)
        for n in (c.n, 1, fc.cpw(depth) + 1, c.n):
            _check(_host(ctx, c.x[:n], inverse), c, n)


@pytest.mark.parametrize("name", ["uniform", "gauss"])
@pytest.mark.parametrize("depth", [8, 4])
def test_forward_scales_by_powers_of_two_exactly(gpu_ctx8, gpu_ctx4, depth, name):
    """forward(2^k x) == 2^k forward(x) for k = -40 and +40: the scaling is exact in every fp64 operation and in the
    final cast as long as every value stays a normal float32, which is asserted from the k = 0 output; no tolerance"""
    ctx = _ctx(gpu_ctx8, gpu_ctx4, depth)
    c = fc.f32_case(name, depth, False)
    base = _dev(ctx, c.x, False)
    assert np.array_equal(base, c.emu)
    f32 = np.finfo(np.float32)
    for k in (-40, 40):
        s = np.float32(2.0 ** k)
        for v in (c.x, base):
            a = np.abs(v[v != 0]).astype(np.float64)
            assert a.min() * 2.0 ** k >= f32.tiny and a.max() * 2.0 ** k <= f32.max
        for out in (_host(ctx, c.x * s, False), _dev(ctx, c.x * s, False)):
            assert np.array_equal(out, base * s)


@pytest.mark.parametrize("depth", [8, 4])
def test_forward_is_odd(gpu_ctx8, gpu_ctx4, depth):
    """forward(-x) == -forward(x): rounding to nearest is symmetric (compared as numbers: an exact zero keeps the
    sign of x - x = +0 on both sides)"""
    ctx = _ctx(gpu_ctx8, gpu_ctx4, depth)
    c = fc.f32_case("uniform", depth, False)
    for out in (_host(ctx, -c.x, False), _dev(ctx, -c.x, False)):
        assert np.array_equal(out, -c.emu)


# ---- fwd64_raster_kernel: the fp64 output of the int32 encode ---------------------------------------------------------

def _check64(d, r):
    """(a), then (b) against dct_ref and against Plan.dct; all are evaluated before any is reported"""
    fails = []
    if not np.array_equal(d, r.emu):
        fails.append(f"(a) {int((d != r.emu).sum())} values differ from the emulation")
    for what, ref in (("dct_ref", r.ref), ("Plan.dct", r.oracle_dct())):
        bad = ~(np.abs(d - ref) <= fc.tol(ref))
        if bad.any():
            fails.append(f"(b) {int(bad.sum())} values further than 1e-9 max(1, |ref|) from {what}")
    assert not fails, "; ".join(fails)


def _encode_dev(ctx, r, want_dct):
    """encode_stacks_dev: (q, the fp64 output or None); the fp64 output lies between canary bands"""
    import torch
    d_fr = torch.from_numpy(r.frames.copy()).cuda()
    q = torch.empty((r.n, r.depth, 8, 8), dtype=torch.int32, device="cuda")
    nbytes = 8 * r.cubes.size
    buf, mid = qc.banded(torch, nbytes, FILL)
    ctx.encode_stacks_dev(d_fr, r.w, r.h, r.stacks, q, mid.view(torch.float64) if want_dct else None)
    ctx.synchronize()
    d, intact = qc.bands_intact(buf, nbytes, FILL)
    assert intact, "a write outside the fp64 output"
    if not want_dct:
        assert (d == FILL).all()
    return q.cpu().numpy(), d.view(np.float64).reshape(r.cubes.shape) if want_dct else None


@pytest.mark.parametrize("w,h,stacks", fc.RASTER_SHAPES)
@pytest.mark.parametrize("depth", [8, 4])
def test_fwd64_raster_host_and_device_entry(gpu_ctx8, gpu_ctx4, depth, w, h, stacks):
    """1, 30, 33, 135 and 512 cubes (the kernel's block is 32): a single cube, an odd cube row with a partial block,
    one cube into a second block, several blocks with a partial last one, and one 255 pixel per cube at every position
    of the cube.  The int32 output is the call's without the fp64 output; under quant_table(12) the fp64 output does
    not change and the int32 output is that table's."""
    ctx = _ctx(gpu_ctx8, gpu_ctx4, depth)
    r = fc.raster_case(w, h, stacks, depth)
    q0 = ctx.encode_stacks(r.frames)
    assert np.array_equal(q0, qc.plan(depth).encode_q(r.frames))
    q, d = ctx.encode_stacks(r.frames, want_dct=True)
    assert np.array_equal(q, q0)
    _check64(d, r)
    q, _ = _encode_dev(ctx, r, False)
    assert np.array_equal(q, q0)
    q, d = _encode_dev(ctx, r, True)
    assert np.array_equal(q, q0)
    _check64(d, r)
    t12 = qc.pkg().quant_table(12, depth)
    ctx.set_quant(t12)
    try:
        q12 = ctx.encode_stacks(r.frames)
        assert np.array_equal(q12, qc.ref_encode(r.frames, t12, depth))
        for q, d in (ctx.encode_stacks(r.frames, want_dct=True), _encode_dev(ctx, r, True)):
            assert np.array_equal(q, q12)
            _check64(d, r)
    finally:
        ctx.set_quant(None)
