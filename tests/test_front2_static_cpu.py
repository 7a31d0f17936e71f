"""front2.hip's static-plan form takes its tile geometry from a constexpr restatement of make_front2_plan()'s arithmetic
(one row of front2_tuned.inc per instantiation).  At the first launch of a shape the constexpr plan is compared, field by
field, with the plan the generic form would be launched with; a difference is WHENET_EINVAL and the kernel never runs.
whenet_front2_static_check() is that comparison as pure host logic: the engine's launch of the row's layer against the row's
static plan with one field moved."""
import pytest

from whenet_hip import _lib

FIELDS = ("H", "Ho", "Cin", "Cexp", "pad", "NTe", "CC", "TH", "TXG", "tiles_x", "tiles_y", "EH", "EWp", "RP", "CP", "off_stage",
          "off_red", "off_sum", "R", "RPse", "ntiles", "chunks", "k", "s", "xs", "threads", "KS", "gated", "lds_bytes")
STATIC_ROWS = (0, 1, 2, 3, 5, 6, 7, 8)        # b2, b3, b4, b5, b7/b8, b9, b10/b11, b12
GENERIC_ROWS = (4, 9, 10)                     # b6, b13-b15, b16: use = 0 in the table


@pytest.mark.parametrize("row", STATIC_ROWS)
def test_static_plan_equals_the_runtime_plan(row):
    assert _lib.load().whenet_front2_static_check(row, -1, 0) == _lib.OK


@pytest.mark.parametrize("row", STATIC_ROWS)
def test_one_field_off_by_one_is_refused(row):
    lib = _lib.load()
    for field, name in enumerate(FIELDS):
        for delta in (1, -1):
            assert lib.whenet_front2_static_check(row, field, delta) == _lib.EINVAL, (row, name, delta)
        assert lib.whenet_front2_static_check(row, field, 0) == _lib.OK, (row, name)


def test_rows_without_a_static_form_and_bad_fields():
    lib = _lib.load()
    for row in GENERIC_ROWS + (-1, 11):
        assert lib.whenet_front2_static_check(row, -1, 0) == _lib.EINVAL, row
    for field in (-2, len(FIELDS)):
        assert lib.whenet_front2_static_check(0, field, 0) == _lib.EINVAL, field
