"""The static-shape forms of the project GEMMs (pw.hip) and of block 6's front kernel (front.hip) take the layer's shape from a
constexpr table instead of the kernel's arguments.  At the first launch of a shape the constexpr shape is compared, field by
field, with what the launch would have passed to the generic form; a difference is WHENET_EINVAL and the kernel never runs.
whenet_pw_static_check() / whenet_front_static_check() are that comparison as pure host logic: the layer as the engine
launches it against the row's static shape with one field moved."""
import pytest

from whenet_hip import _lib

PW_FIELDS = ("K", "N", "HW", "KS", "NTILES", "NCH", "family", "B2", "GM", "RES", "lay", "np", "R", "RP")
# b2, b3, b4, b5, b6, b7/b8, b9, b10/b11, b12, b13-15, b16: every row's constexpr shape is held to the layer's launch, also rows
# 3, 4, 7 and 8, whose static form is not built (use = 0 in the table: more VGPRs than their generic kernel, or slower)
PW_ROWS = tuple(range(11))
FRONT_FIELDS = ("H", "Ho", "Cin", "Cexp", "pad", "KSe", "NTe", "CC", "TH", "NSX", "tiles_x", "tiles_y", "EH", "EW", "EP", "w_off",
                "R", "RP", "ntiles", "chunks", "k", "s", "threads", "lds_bytes")


@pytest.mark.parametrize("row", PW_ROWS)
def test_pw_static_shape_equals_the_launch(row):
    assert _lib.load().whenet_pw_static_check(row, -1, 0) == _lib.OK


@pytest.mark.parametrize("row", PW_ROWS)
def test_pw_one_field_off_by_one_is_refused(row):
    lib = _lib.load()
    for field, name in enumerate(PW_FIELDS):
        for delta in (1, -1):
            assert lib.whenet_pw_static_check(row, field, delta) == _lib.EINVAL, (row, name, delta)
        assert lib.whenet_pw_static_check(row, field, 0) == _lib.OK, (row, name)


def test_pw_bad_rows_and_fields():
    lib = _lib.load()
    for row in (-1, 11):
        assert lib.whenet_pw_static_check(row, -1, 0) == _lib.EINVAL, row
    for field in (-2, len(PW_FIELDS)):
        assert lib.whenet_pw_static_check(0, field, 0) == _lib.EINVAL, field


def test_front_static_shape_equals_the_launch():
    assert _lib.load().whenet_front_static_check(0, -1, 0) == _lib.OK


def test_front_one_field_off_by_one_is_refused():
    lib = _lib.load()
    for field, name in enumerate(FRONT_FIELDS):
        for delta in (1, -1):
            assert lib.whenet_front_static_check(0, field, delta) == _lib.EINVAL, (name, delta)
        assert lib.whenet_front_static_check(0, field, 0) == _lib.OK, name


def test_front_bad_rows_and_fields():
    lib = _lib.load()
    for row in (-1, 1):
        assert lib.whenet_front_static_check(row, -1, 0) == _lib.EINVAL, row
    for field in (-2, len(FRONT_FIELDS)):
        assert lib.whenet_front_static_check(0, field, 0) == _lib.EINVAL, field
