"""CPU: ssim_windows_ref, the SSIM probe's definition in numpy (include/dct3d.h): the windows' count and
shape, the bounds the int64 / fp64 arithmetic rests on, agreement with the textbook float SSIM on the same windows,
and one window worked out by hand.  Nothing here needs a device or the library."""
from fractions import Fraction

import numpy as np
import pytest

SIZES = [(1, 1), (4, 4), (5, 3), (8, 8), (9, 4), (61, 45), (64, 64)]  # (w, h)
ONE = 1 << 24


def _windows(w, h):
    nbx, nby = -(-w // 4), -(-h // 4)
    return max(nbx - 1, 1), max(nby - 1, 1)


def _contents(w, h):
    rng = np.random.default_rng(w * 1000 + h)
    y, x = np.ogrid[:h, :w]
    chk = (255 * ((x + y) & 1)).astype(np.uint8)
    noise = rng.integers(0, 256, (h, w), dtype=np.uint8)
    return {
        "zeros": (np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)),
        "0-255": (np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8)),
        "255-255": (np.full((h, w), 255, np.uint8), np.full((h, w), 255, np.uint8)),
        "chk-inverse": (chk, 255 - chk),
        "noise-noise": (noise, rng.integers(0, 256, (h, w), dtype=np.uint8)),
        "noise-near": (noise, np.clip(noise.astype(np.int16) + rng.integers(-6, 7, (h, w)), 0, 255).astype(np.uint8)),
        "noise-inverse": (noise, 255 - noise),
    }


@pytest.mark.parametrize("w,h", SIZES)
def test_identical_planes_give_one_in_every_window(pkg, w, h):
    for name, (x, _) in _contents(w, h).items():
        v = pkg.ssim_windows_ref(x, x)
        assert v.dtype == np.int64 and (v == ONE).all(), name


@pytest.mark.parametrize("w,h", SIZES)
def test_window_counts_and_shapes(pkg, w, h):
    nwx, nwy = _windows(w, h)
    x, y = _contents(w, h)["noise-near"]
    assert pkg.ssim_windows_ref(x, y).shape == (nwy, nwx)
    stack = np.stack([x, y, x])
    v = pkg.ssim_windows_ref(np.stack([stack, stack]), np.stack([stack[::-1], stack]))
    assert v.shape == (2, 3, nwy, nwx)
    assert np.array_equal(v[0, 0], pkg.ssim_windows_ref(x, x)) and np.array_equal(v[0, 1], pkg.ssim_windows_ref(y, y))
    assert np.array_equal(v[1, 1], np.full((nwy, nwx), ONE))
    assert {(1, 1): (1, 1), (4, 4): (1, 1), (5, 3): (1, 1), (8, 8): (1, 1), (9, 4): (2, 1), (61, 45): (15, 11),
            (64, 64): (15, 15)}[(w, h)] == (nwx, nwy)
    for bad in ((x, y[:, :-1]) if w > 1 else (x, y[None]), (x.astype(np.int32), y), (x[0], y[0])):
        with pytest.raises(ValueError):
            pkg.ssim_windows_ref(*bad)


@pytest.mark.parametrize("w,h", SIZES)
def test_bounds(pkg, w, h):
    """|A|, |B|, C, D < 2^53 (their conversion to fp64 is exact), C, D > 0, A B <= C D (|s| <= 1) and |v| <= 2^24"""
    for name, (x, y) in _contents(w, h).items():
        v, A, B, Cc, D = pkg.ssim_windows_ref(x, y, _parts=True)
        for t in (A, B, Cc, D):
            assert t.dtype == np.int64 and (np.abs(t) < (1 << 53)).all(), name
        assert (Cc > 0).all() and (D > 0).all(), name
        assert (np.abs(v) <= ONE).all(), name
        for a, b, c, d in zip(A.ravel(), B.ravel(), Cc.ravel(), D.ravel()):
            assert abs(int(a) * int(b)) <= int(c) * int(d), name


def _textbook(x, y):
    """the float SSIM with population moments over the same windows: (2 mx my + c1)(2 cov + c2) / ((mx^2 + my^2 + c1)
    (vx + vy + c2)), c1 = (0.01 255)^2, c2 = (0.03 255)^2"""
    h, w = x.shape
    nwx, nwy = _windows(w, h)
    out = np.empty((nwy, nwx))
    c1, c2 = 6.5025, 58.5225
    for j in range(nwy):
        for i in range(nwx):
            a = x[4 * j:4 * j + 8, 4 * i:4 * i + 8].astype(np.float64).ravel()
            b = y[4 * j:4 * j + 8, 4 * i:4 * i + 8].astype(np.float64).ravel()
            ma, mb = a.mean(), b.mean()
            va, vb, cov = ((a - ma) ** 2).mean(), ((b - mb) ** 2).mean(), ((a - ma) * (b - mb)).mean()
            out[j, i] = (2 * ma * mb + c1) * (2 * cov + c2) / ((ma * ma + mb * mb + c1) * (va + vb + c2))
    return out


@pytest.mark.parametrize("w,h", SIZES)
def test_agrees_with_the_textbook_float_ssim(pkg, w, h):
    for name, (x, y) in _contents(w, h).items():
        v = pkg.ssim_windows_ref(x, y)
        assert np.abs(v / ONE - _textbook(x, y)).max() <= 2.0 ** -20, name


def test_one_window_by_hand(pkg):
    """5 x 3: one window of n = 15 samples.  x = 10 everywhere, y = 10 but for one sample of 25:
    Sx = 150, Sy = 165, Sxx = 1500, Syy = 2025, Sxy = 1650."""
    x = np.full((3, 5), 10, np.uint8)
    y = x.copy()
    y[1, 4] = 25  # in the second block column: the window sums two blocks
    n, Sx, Sy, Sxx, Syy, Sxy = 15, 150, 165, 1500, 2025, 1650
    A = 20000 * Sx * Sy + 65025 * n * n
    B = 20000 * (n * Sxy - Sx * Sy) + 585225 * n * n
    Cc = 10000 * (Sx * Sx + Sy * Sy) + 65025 * n * n
    D = 10000 * (n * Sxx - Sx * Sx + n * Syy - Sy * Sy) + 585225 * n * n
    assert (A, B, Cc, D) == (509630625, 131675625, 511880625, 163175625)
    exact = Fraction(A * B, Cc * D)
    v, a, b, c, d = pkg.ssim_windows_ref(x, y, _parts=True)
    assert (int(a[0, 0]), int(b[0, 0]), int(c[0, 0]), int(d[0, 0])) == (A, B, Cc, D)
    assert v.shape == (1, 1)
    # the exact quotient lies well inside a cell of the 2^-24 grid: the three fp64 roundings cannot move the floor
    cell = exact * ONE
    assert min(cell - int(cell), int(cell) + 1 - cell) > Fraction(1, 1 << 20)
    assert int(v[0, 0]) == int(cell) == 13478973  # s = 0.99560 x 0.80696 = 0.80341


def test_ssim_mean(pkg):
    assert pkg.ssim_mean(ONE * 7, 7) == 1.0
    assert pkg.ssim_mean(-ONE * 3, 6) == -0.5
    assert pkg.ssim_mean(np.int64(ONE), np.int64(4)) == 0.25
    with pytest.raises(ValueError):
        pkg.ssim_mean(1, 0)
