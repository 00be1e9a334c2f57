"""CPU: the numpy definitions of 4:2:0 chroma subsampling (DCT3D_CHROMA_420; dct3d.h) -- chroma_size,
subsample_420, upsample_420, rgb_to_ycbcr420, ycbcr420_to_rgb -- which the GPU tests (test_gpu_c420.py) take as their
reference.  Nothing here needs a device."""
import numpy as np
import pytest

SIZES = [(1, 1), (2, 2), (5, 3), (13, 11), (16, 16), (17, 16), (61, 27)]


def test_chroma_size(pkg):
    assert [pkg.chroma_size(n, n) for n in (1, 2, 15, 16, 17)] == [(1, 1), (1, 1), (8, 8), (8, 8), (9, 9)]
    assert pkg.chroma_size(17, 2) == (9, 1) and pkg.chroma_size(1366, 24) == (683, 12)
    for bad in ((0, 4), (4, 0), (-1, 4)):
        with pytest.raises(ValueError):
            pkg.chroma_size(*bad)


@pytest.mark.parametrize("w,h", SIZES)
def test_subsample_of_upsample_is_the_identity(pkg, w, h):
    cw, ch = pkg.chroma_size(w, h)
    c = np.random.default_rng(w * 100 + h).integers(0, 256, (3, ch, cw), dtype=np.uint8)
    up = pkg.upsample_420(c, w, h)
    assert up.shape == (3, h, w) and up.dtype == np.uint8
    assert np.array_equal(pkg.subsample_420(up), c)
    # replication: every pixel is its chroma sample
    yy, xx = np.mgrid[:h, :w]
    assert np.array_equal(up, c[:, yy >> 1, xx >> 1])


@pytest.mark.parametrize("w,h", SIZES)
def test_constant_and_grey(pkg, w, h):
    """a plane of 128 stays 128; grey frames (R = G = B) have chroma 128 and keep their luma"""
    assert np.array_equal(pkg.subsample_420(np.full((2, h, w), 128, np.uint8)), np.full((2,) + pkg.chroma_size(w, h)[::-1], 128))
    g = np.random.default_rng(7).integers(0, 256, (4, h, w), dtype=np.uint8)
    y, cb, cr = pkg.rgb_to_ycbcr420(np.stack([g] * 3, axis=-1))
    assert np.array_equal(y, g) and (cb == 128).all() and (cr == 128).all()
    assert cb.shape == cr.shape == (4,) + pkg.chroma_size(w, h)[::-1]


@pytest.mark.parametrize("w,h", SIZES)
def test_planes_constant_on_aligned_blocks(pkg, w, h):
    """frames constant on aligned 2 x 2 blocks lose nothing: rgb_to_ycbcr420 followed by upsample_420 is rgb_to_ycbcr,
    and ycbcr420_to_rgb of it is ycbcr_to_rgb of rgb_to_ycbcr"""
    cw, ch = pkg.chroma_size(w, h)
    small = np.random.default_rng(w + 31 * h).integers(0, 256, (2, ch, cw, 3), dtype=np.uint8)
    fr = np.repeat(np.repeat(small, 2, axis=1), 2, axis=2)[:, :h, :w]
    t = pkg.rgb_to_ycbcr(fr)
    y, cb, cr = pkg.rgb_to_ycbcr420(fr)
    assert np.array_equal(y, t[..., 0])
    assert np.array_equal(pkg.upsample_420(cb, w, h), t[..., 1]) and np.array_equal(pkg.upsample_420(cr, w, h), t[..., 2])
    assert np.array_equal(pkg.ycbcr420_to_rgb(y, cb, cr), pkg.ycbcr_to_rgb(t))


@pytest.mark.parametrize("w,h", SIZES)
def test_box_sum_against_a_float_mean(pkg, w, h):
    """the box sum is the mean of the four (edge-replicated) samples, within 0.5; and it is S after T: the subsampled
    planes of rgb_to_ycbcr420 are subsample_420 of rgb_to_ycbcr's"""
    p = np.random.default_rng(3 * w + h).integers(0, 256, (3, h, w), dtype=np.uint8)
    pad = np.pad(p, ((0, 0), (0, h % 2), (0, w % 2)), mode="edge").astype(np.float64)
    mean = (pad[:, 0::2, 0::2] + pad[:, 0::2, 1::2] + pad[:, 1::2, 0::2] + pad[:, 1::2, 1::2]) / 4.0
    got = pkg.subsample_420(p)
    assert got.dtype == np.uint8 and got.shape == mean.shape
    assert np.abs(got.astype(np.float64) - mean).max() <= 0.5
    assert np.array_equal(got, np.floor(mean + 0.5))  # halves round up: (s + 2) >> 2
    fr = np.random.default_rng(5).integers(0, 256, (2, h, w, 3), dtype=np.uint8)
    t = pkg.rgb_to_ycbcr(fr)
    y, cb, cr = pkg.rgb_to_ycbcr420(fr)
    assert np.array_equal(cb, pkg.subsample_420(t[..., 1])) and np.array_equal(cr, pkg.subsample_420(t[..., 2]))
    assert np.array_equal(pkg.ycbcr420_to_rgb(y, cb, cr),
                          pkg.ycbcr_to_rgb(np.stack((y, pkg.upsample_420(cb, w, h), pkg.upsample_420(cr, w, h)), axis=-1)))


def test_shapes_are_checked(pkg):
    with pytest.raises(ValueError):
        pkg.upsample_420(np.zeros((2, 3, 3), np.uint8), 5, 3)  # (5, 3) has chroma planes of 2 x 3
    with pytest.raises(ValueError):
        pkg.subsample_420(np.zeros(4, np.uint8))
    with pytest.raises(ValueError):
        pkg.rgb_to_ycbcr420(np.zeros((4, 4, 2), np.uint8))
