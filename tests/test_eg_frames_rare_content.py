"""CPU: the content the fused stream encode's rare-path test relies on (tests/test_gpu_eg_frames.py, the 29 x 7,
48-stack content of test_gpu_edge._rare_content) does reach the rare path: the host emulation of the kernel's
fp32 arithmetic (tests/native/emulate_encode.cpp) leaves at least one coefficient of the edge-padded raster open
at each depth, grey and in every channel of the packed RGB24 content.  The fused kernel has no second
certificate, so each of them is an exact replay there."""
import numpy as np
import pytest

from test_emulation import emu, run  # noqa: F401  (emu: the module fixture that builds the emulation)
from test_gpu_edge import _rare_content


@pytest.mark.parametrize("depth", [8, 4])
def test_rare_content_leaves_coefficients_open(emu, pkg, oracle, depth):  # noqa: F811
    rgb = _rare_content(pkg, depth, 3)
    assert np.array_equal(rgb[..., 0], _rare_content(pkg, depth, 1))  # the grey content is the red plane
    for ch in range(3):
        pad = np.ascontiguousarray(pkg.pad_frames(np.ascontiguousarray(rgb[..., ch])))
        _, fl, _, _, _ = run(emu, pkg, oracle.to_cubes(pad, 8, 8, depth), depth)
        print(f"depth {depth} channel {ch}: {int(fl.sum())} open coefficients of {fl.size}")
        assert fl.sum() > 0, (depth, ch)
