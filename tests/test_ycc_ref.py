"""CPU: the definition of the YCbCr colour transform (rgb_to_ycbcr, ycbcr_to_rgb; dct3d.h) over all 2^24
inputs of each direction: ranges, grey pixels, the distance to the real-valued JFIF formulas, the clamp being live,
the round trip, and a restatement with plain Python integers."""
import functools

import numpy as np

BOUND = 0.502  # the fixed-point coefficients' error on top of the rounding's half (measured: 0.5010 and 0.5015)


@functools.lru_cache(maxsize=None)
def _all_triples():
    """every (a, b, c) in [0, 255]^3 as uint8 [2^24, 3] (read-only)"""
    i = np.arange(1 << 24, dtype=np.uint32)
    t = np.stack((i >> 16, (i >> 8) & 255, i & 255), axis=-1).astype(np.uint8)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def _forward(pkg_name):
    import importlib
    out = importlib.import_module(pkg_name).rgb_to_ycbcr(_all_triples())
    out.setflags(write=False)
    return out


def _real_forward(rgb):
    r, g, b = (rgb[:, i].astype(np.float64) for i in range(3))
    return np.stack((0.299 * r + 0.587 * g + 0.114 * b,
                     128.0 - 0.168735892 * r - 0.331264108 * g + 0.5 * b,
                     128.0 + 0.5 * r - 0.418687589 * g - 0.081312411 * b), axis=-1)


def _real_inverse(ycc):
    y, u, v = ycc[:, 0].astype(np.float64), ycc[:, 1].astype(np.float64) - 128.0, ycc[:, 2].astype(np.float64) - 128.0
    return np.stack((y + 1.402 * v, y - 0.344136286 * u - 0.714136286 * v, y + 1.772 * u), axis=-1)


def test_forward_range_dtype_and_numerators(pkg):
    rgb = _all_triples()
    out = _forward(pkg.__name__)
    assert out.dtype == np.uint8 and out.shape == rgb.shape
    a = rgb.astype(np.int64)
    r, g, b = a[:, 0], a[:, 1], a[:, 2]
    nums = (19595 * r + 38470 * g + 7471 * b + 32768,
            -11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767,
            32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767)
    for ch, num in enumerate(nums):
        assert num.min() >= 0 and num.max() <= (1 << 24) - 1  # [0, 255] with no clamp; exact in 24-bit multiply-adds
        assert np.array_equal(out[:, ch], num >> 16)           # (nothing was lost in the cast to uint8)
        assert out[:, ch].min() == 0 and out[:, ch].max() == 255


def test_grey_pixels_map_to_v_128_128(pkg):
    v = np.arange(256, dtype=np.uint8)
    grey = np.stack((v, v, v), axis=-1)
    want = np.stack((v, np.full(256, 128, np.uint8), np.full(256, 128, np.uint8)), axis=-1)
    assert np.array_equal(pkg.rgb_to_ycbcr(grey), want)


def test_forward_is_within_the_bound_of_the_real_formulas(pkg):
    d = np.abs(_forward(pkg.__name__).astype(np.float64) - _real_forward(_all_triples())).max(axis=0)
    print("forward distance per channel:", d)
    assert (d <= BOUND).all(), d


def test_inverse_before_the_clamp_is_within_the_bound_and_the_clamp_is_live(pkg):
    ycc = _all_triples()
    pre = pkg.ycbcr_to_rgb_unclamped(ycc)
    d = np.abs(pre.astype(np.float64) - _real_inverse(ycc)).max(axis=0)
    print("inverse pre-clamp distance per channel:", d, "range:", pre.min(axis=0), pre.max(axis=0))
    assert (d <= BOUND).all(), d
    assert (pre.min(axis=0) < 0).all() and (pre.max(axis=0) > 255).all()  # every channel leaves [0, 255] on both sides
    out = pkg.ycbcr_to_rgb(ycc)
    assert out.dtype == np.uint8 and np.array_equal(out, np.clip(pre, 0, 255))


def test_round_trip_error_is_exactly_one_at_its_maximum(pkg):
    rgb = _all_triples()
    back = pkg.ycbcr_to_rgb(_forward(pkg.__name__))
    err = np.abs(back.astype(np.int16) - rgb.astype(np.int16)).max(axis=0)
    assert err.tolist() == [1, 1, 1]


def _forward_int(r, g, b):
    return ((19595 * r + 38470 * g + 7471 * b + 32768) >> 16,
            (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16,
            (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16)


def _inverse_int(y, cb, cr):
    u, v = cb - 128, cr - 128
    clamp = lambda x: min(max(x, 0), 255)
    return (clamp(y + ((91881 * v + 32768) >> 16)), clamp(y + ((-22554 * u - 46802 * v + 32768) >> 16)),
            clamp(y + ((116130 * u + 32768) >> 16)))


def test_equal_to_plain_python_integers_on_a_seeded_sample(pkg):
    t = np.random.default_rng(20261020).integers(0, 256, size=(10**4, 3)).astype(np.uint8)
    f, i = pkg.rgb_to_ycbcr(t), pkg.ycbcr_to_rgb(t)
    for k in range(t.shape[0]):
        a = tuple(int(x) for x in t[k])
        assert tuple(f[k]) == _forward_int(*a) and tuple(i[k]) == _inverse_int(*a), a


def test_any_leading_shape_and_a_last_axis_of_three(pkg):
    t = np.random.default_rng(7).integers(0, 256, size=(2, 5, 4, 3)).astype(np.uint8)
    assert np.array_equal(pkg.rgb_to_ycbcr(t).reshape(-1, 3), pkg.rgb_to_ycbcr(t.reshape(-1, 3)))
    assert np.array_equal(pkg.ycbcr_to_rgb(t).reshape(-1, 3), pkg.ycbcr_to_rgb(t.reshape(-1, 3)))
    assert pkg.rgb_to_ycbcr(t[0, 0, 0]).shape == (3,)
    for bad in (np.zeros((4, 2), np.uint8), np.zeros((), np.uint8)):
        for f in (pkg.rgb_to_ycbcr, pkg.ycbcr_to_rgb):
            try:
                f(bad)
            except ValueError:
                continue
            raise AssertionError("a last axis that is not 3 must be refused")
