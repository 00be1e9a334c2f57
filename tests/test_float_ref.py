"""CPU: the two references test_gpu_float.py holds the float kernels to (float_common.py), checked against each other
and against the oracle before any device is asked.

  * dct_ref, the long-double cosine-definition DCT, against the oracle's Java-semantics Plan.dct / Plan.idct and
    against orthonormality;
  * the host emulation of cube_f32_kernel and fwd64_raster_kernel (tests/native/emulate_float.cpp) against dct_ref, on
    every unit impulse and on every input of the GPU module, within the project's 1e-9 max(1, |ref|).  The largest
    absolute error over the pixel-range inputs is printed (pytest -s) and recorded in DESIGN "Float outputs": it is the
    evidence for that bound, and comes from this comparison alone;
  * the preconditions the GPU cases state about their inputs."""
import numpy as np
import pytest

import float_common as fc
import quant_common as qc


@pytest.mark.parametrize("N", [8, 4])
def test_dct_matrix_is_orthonormal(N):
    m = fc.dct_matrix(N)
    assert m.dtype == np.longdouble and np.finfo(np.longdouble).eps < 1e-18  # an x87 or wider long double
    assert np.abs(m @ m.T - np.eye(N)).max() <= 1e-15
    assert np.abs(m.T @ m - np.eye(N)).max() <= 1e-15


@pytest.mark.parametrize("kind", ["ramp", "uniform"])
@pytest.mark.parametrize("depth", [8, 4])
def test_dct_ref_matches_the_oracle(oracle, depth, kind):
    """Plan.dct and Plan.idct (the Java fold: another summation order in fp64) within 1e-9 max(1, |ref|) of dct_ref;
    the inverse after the clamp"""
    plan = qc.plan(depth)
    fr = fc._frames(24, 16, 3, depth, kind)
    ref = fc.dct_ref(oracle.to_cubes(fr, 8, 8, depth), depth, False)
    got = oracle.to_cubes(plan.dct(fr), 8, 8, depth)
    assert np.all(np.abs(got - ref) <= fc.tol(ref))
    deq = oracle.dequantize(plan.encode_q(fr), 24, 16, fr.shape[0], 8, 8, depth)
    inv = np.clip(fc.dct_ref(oracle.to_cubes(deq, 8, 8, depth), depth, True), 0.0, 255.0)
    got = oracle.to_cubes(plan.idct(deq), 8, 8, depth)
    assert np.all(np.abs(got - inv) <= fc.tol(inv))


def test_dct_ref_round_trip():
    """the inverse is the transpose: inverse(forward(x)) = x to long-double accuracy"""
    x = np.random.default_rng(5).normal(0.0, 100.0, size=(7, 4, 8, 8))
    back = fc.dct_ref(fc.dct_ref(x, 4, False), 4, True)
    assert np.abs(back - x).max() <= 1e-12


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("depth", [8, 4])
def test_emulation_on_unit_impulses(depth, inverse):
    """every basis element alone: each entry of the butterflies' matrices, forward and inverse, against the cosines"""
    x = fc._impulses(depth, 1.0).astype(np.float32)
    out, pre = fc.emu_cube_f32(x, depth, inverse, want_pre=True)
    ref = fc.dct_ref(x, depth, inverse)
    err = np.abs(pre - ref)
    print(f"impulses depth {depth} inverse {inverse}: max |emulation - dct_ref| = {err.max():.3e}")
    assert np.all(err <= fc.tol(ref))
    assert err.max() <= 1e-15  # |values| < 0.36: a handful of roundings of numbers below 1
    exp = np.clip(ref, 0.0, 255.0) if inverse else ref
    assert np.array_equal(out, np.clip(pre, 0.0, 255.0).astype(np.float32) if inverse else pre.astype(np.float32))
    assert fc.in_f32_window(out, exp)


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("depth", [8, 4])
def test_emulation_within_bound_on_the_gpu_inputs(depth, inverse):
    """every input of test_gpu_float.py's cube_f32 cases: the emulation's fp64 values within 1e-9 max(1, |ref|) of
    dct_ref, its float32 output inside the window the device's output is held to"""
    worst = 0.0
    for name in fc.case_names(depth, inverse):
        c = fc.f32_case(name, depth, inverse)
        out, pre = fc.emu_cube_f32(c.x, depth, inverse, want_pre=True)
        assert np.array_equal(out, c.emu)
        err = np.abs(pre - c.ref)
        assert np.all(err <= fc.tol(c.ref)), name
        assert fc.in_f32_window(c.emu, c.expected()), name
        if name in fc.PIXEL_RANGE[inverse]:
            worst = max(worst, float(err.max()))
    print(f"cube_f32 depth {depth} inverse {inverse}: max |emulation - dct_ref| on pixel-range input = {worst:.3e}")
    assert worst <= 1e-11  # two orders inside the bound at |ref| = 1


@pytest.mark.parametrize("depth", [8, 4])
def test_raster_emulation_within_bound(depth):
    """the inputs of the fwd64_raster_kernel cases: the emulation within the bound of dct_ref, and the oracle too"""
    worst = 0.0
    for shape in fc.RASTER_SHAPES:
        r = fc.raster_case(*shape, depth)
        assert r.n == shape[0] // 8 * (shape[1] // 8) * shape[2]
        err = np.abs(r.emu - r.ref)
        assert np.all(err <= fc.tol(r.ref)), shape
        assert np.all(np.abs(r.oracle_dct() - r.ref) <= fc.tol(r.ref)), shape
        worst = max(worst, float(err.max()))
    print(f"fwd64 depth {depth}: max |emulation - dct_ref| = {worst:.3e}")
    assert worst <= 1e-11
    one = fc.raster_case(64, 64, 8, depth)  # every position of the cube holds the one pixel of some cube
    flat = one.cubes.reshape(512, -1)
    assert (np.count_nonzero(flat, axis=1) == 1).all() and flat.max() == 255
    assert set(np.argmax(flat, axis=1).tolist()) == set(range(64 * depth))


@pytest.mark.parametrize("depth", [8, 4])
def test_what_the_equality_adds(depth):
    """The same passes in another order (X, Y, Z) are a different rounding sequence of the same transform: well inside
    the tolerance, and not equal.  fwd64's fp64 output shows it in thousands of values; cube_f32's fp64 values differ
    too, but its float32 outputs do not on any input here (a difference of 1e-13 moves a float32 rounding of values
    up to 3000 with probability ~1e-9 per value): there the equality pins the clamp, the cast and the layout, and
    the window already stands at the float rounding."""
    r = fc.raster_case(72, 40, 3, depth)
    alt = fc.emu_fwd64(r.cubes, depth, order=1)
    assert np.all(np.abs(alt - r.ref) <= fc.tol(r.ref))
    assert np.count_nonzero(alt != r.emu) > 1000
    c = fc.f32_case("uniform", depth, False)
    out, pre = fc.emu_cube_f32(c.x, depth, False, want_pre=True)
    out1, pre1 = fc.emu_cube_f32(c.x, depth, False, order=1, want_pre=True)
    assert np.count_nonzero(pre1 != pre) > 1000 and fc.in_f32_window(out1, c.ref)


@pytest.mark.parametrize("depth", [8, 4])
def test_preconditions_of_the_gpu_cases(depth):
    """what test_gpu_float.py says about its inputs, from dct_ref alone"""
    b = fc.f32_case("basis", depth, True)  # unclamped: every entry of the inverse butterflies is compared as computed
    assert b.n == 64 * depth and 0.0 < b.ref.min() and b.ref.max() < 255.0
    u = fc.f32_case("uniform", depth, True)  # both clamp arms live
    assert u.ref.min() < -1.0 and u.ref.max() > 256.0
    p = fc.f32_case("pool", depth, True)
    assert p.ref.min() < -1.0 and p.ref.max() > 256.0
    k = fc.f32_case("const", depth, True)
    assert np.allclose(k.ref[:, 0, 0, 0], [0.0, 255.0, -3.0, 300.0, 254.5], atol=1e-3)
    t, cw = fc.tile(depth), fc.cpw(depth)
    counts = fc.tail_counts(depth)
    assert sorted({-(-n // t) for n in counts}) == [1, 2, 8, 9, 16, 18] and max(counts) == p.n
    assert any(n % cw for n in counts if -(-n // t) % 8) and any(n % cw == 0 for n in counts)
    for name in ("basis255", "basis-1000.5"):  # the impulses, then a partial tile
        f = fc.f32_case(name, depth, False)
        assert f.n == 64 * depth + (3 if depth == 8 else 5) and f.n % cw
        flat = f.x[:64 * depth].reshape(64 * depth, -1)
        assert (np.count_nonzero(flat, axis=1) == 1).all() and (np.argmax(np.abs(flat), axis=1) == np.arange(64 * depth)).all()
    for name in ("uniform", "ramp"):
        assert fc.f32_case(name, depth, False).n == (18 if depth == 8 else 30)
    # the scalings by 2^+-40 stay normal float32 numbers on both sides (exact zeros stay zeros)
    for name in ("uniform", "gauss"):
        c = fc.f32_case(name, depth, False)
        for v in (np.abs(c.x[c.x != 0]), np.abs(c.emu[c.emu != 0])):
            assert v.min() * 2.0 ** -40 >= np.finfo(np.float32).tiny and v.max() * 2.0 ** 40 <= np.finfo(np.float32).max
