"""CPU: which translation unit holds which kernel variant (csrc/dct3d_variant.h), compiled with g++
(tests/native/variant_check.cpp runs the real header) and compared with a table written out here, and the picks
that turn the runtime's four values into template arguments."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RASTER, STREAM = 0, 1
UNITS = {RASTER: ["dct3d_kernels.hip", "dct3d_rgb.hip", "dct3d_edge.hip", "dct3d_quant.hip"],
         STREAM: ["dct3d_kernels.hip", "dct3d_eg_frames.hip", "dct3d_quant_eg.hip"]}
# (px, edge, qt) -> the unit, at either depth: what the runtime's conditionals chose before there was a variant
# header (encode_dev / decode_dev: the table kernels if the context uses its table, else by 2 px + edge; the
# stream encode chain: the table kernels, else the plain grey kernel, else the frames unit; the stream decode:
# RGB to the frames unit or its table twin, grey to the table unit, else the cropping one, else the plain one).
HOLDER = {
    RASTER: {(1, 0, 0): "dct3d_kernels.hip", (1, 1, 0): "dct3d_edge.hip",
             (3, 0, 0): "dct3d_rgb.hip", (3, 1, 0): "dct3d_edge.hip",
             (1, 0, 1): "dct3d_quant.hip", (1, 1, 1): "dct3d_quant.hip",
             (3, 0, 1): "dct3d_quant.hip", (3, 1, 1): "dct3d_quant.hip"},
    STREAM: {(1, 0, 0): "dct3d_kernels.hip", (1, 1, 0): "dct3d_eg_frames.hip",
             (3, 0, 0): "dct3d_eg_frames.hip", (3, 1, 0): "dct3d_eg_frames.hip",
             (1, 0, 1): "dct3d_quant_eg.hip", (1, 1, 1): "dct3d_quant_eg.hip",
             (3, 0, 1): "dct3d_quant_eg.hip", (3, 1, 1): "dct3d_quant_eg.hip"},
}
VALID = list(itertools.product((8, 4), (1, 3), (0, 1), (0, 1)))
# one axis just outside its values, the others valid
OUTSIDE = ([(D, 1, 0, 0) for D in (2, 16)] + [(8, px, 0, 0) for px in (0, 2)] + [(8, 1, 2, 0), (8, 1, 0, 2)] +
           [(16, 3, 1, 1), (4, 2, 1, 1), (4, 3, 2, 1), (4, 3, 1, 2)])


@pytest.fixture(scope="module")
def vlib(tmp_path_factory):
    out = tmp_path_factory.mktemp("variant") / "libvariant.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC",
                    "-I", os.path.join(REPO, "3ddctvideoencoding_amd", "csrc"),
                    os.path.join(REPO, "tests", "native", "variant_check.cpp"), "-o", str(out)], check=True)
    L = C.CDLL(str(out))
    for f in (L.variant_held_by, L.variant_index, L.variant_routed_to):
        f.argtypes = [C.c_int] * 5
    L.variant_pick4.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_int)] * 2
    L.variant_pick3.argtypes = [C.c_int] * 3 + [C.POINTER(C.c_int)] * 2
    L.variant_groups.argtypes = [C.c_int] * 2
    return L


def test_the_table_names_every_variant():
    assert len(VALID) == 16
    for family in (RASTER, STREAM):
        assert sorted(HOLDER[family]) == sorted({v[1:] for v in VALID})
        assert set(HOLDER[family].values()) == set(UNITS[family])


@pytest.mark.parametrize("family", [RASTER, STREAM])
def test_each_variant_is_held_by_exactly_the_unit_of_the_table(vlib, family):
    for D, px, edge, qt in VALID:
        want = UNITS[family].index(HOLDER[family][(px, edge, qt)])
        assert vlib.variant_held_by(family, D, px, edge, qt) == 1 << want, (D, px, edge, qt)  # that unit and no other
        assert vlib.variant_index(family, D, px, edge, qt) == want
        assert vlib.variant_routed_to(family, D, px, edge, qt) == want  # (one call of the router's functor)


def test_with_variant_hands_over_the_four_values(vlib):
    out, said = (C.c_int * 4)(), C.c_int()
    for v in VALID:
        out[:] = [-1] * 4
        assert vlib.variant_pick4(*v, out, C.byref(said)) == 1
        assert tuple(out) == v and said.value == 1
        out[:] = [-1] * 4
        assert vlib.variant_pick3(*v[:3], out, C.byref(said)) == 1
        assert tuple(out)[:3] == v[:3] and said.value == 1


def test_values_outside_an_axis_call_nothing_and_say_so(vlib):
    out, said = (C.c_int * 4)(), C.c_int(7)
    for v in OUTSIDE:
        assert vlib.variant_pick4(*v, out, C.byref(said)) == 0, v
        assert said.value == 0, v
    for v in [v[:3] for v in OUTSIDE if v[3] in (0, 1)]:
        assert vlib.variant_pick3(*v, out, C.byref(said)) == 0, v
        assert said.value == 0, v


def test_group_pick(vlib):
    """the grey stream decode's groups per wave: 1 | 2 | 4 | 8 in the plain unit (any other value: 8), 8 elsewhere"""
    asked = [1, 2, 4, 8, 0, 3, 5, 16, -1]
    assert [vlib.variant_groups(0, n) for n in asked] == [1, 2, 4, 8, 8, 8, 8, 8, 8]
    for unit in (1, 2):
        assert [vlib.variant_groups(unit, n) for n in asked] == [8] * len(asked)
