"""rt_hip_lights_from_spec (include/rt_hip.h; rt_amd/csrc/lights.cpp): an emission table from a text.  Host-only — the library is loaded,
no device is touched.  Every well-formed shape gives the table one expects; every malformed one gives RT_HIP_INVALID_ARGUMENT with the
offending item in the message and leaves the output alone."""
import ctypes as C

import numpy as np
import pytest

import rt_amd
from rt_amd import capi
from tests import light_reference as light_ref

NAMES = ["ground", "lamp", "clay", "lamp", "glass"]  # (two materials share a name)
INVALID_ARGUMENT = 1


def table(spec, names=NAMES, n=None):
    return rt_amd.renderer.lights_from_spec(spec, names, n)


def rows(**lit):
    out = np.zeros((len(NAMES), 3), dtype=np.float32)
    for index, rgb in lit.items():
        out[int(index[1:])] = rgb
    return out


def test_index_keys():
    assert np.array_equal(table("1=4,3.5,2"), rows(m1=(4, 3.5, 2)))
    assert np.array_equal(table("0=1,0,0;4=0,0,0.25"), rows(m0=(1, 0, 0), m4=(0, 0, 0.25)))
    assert np.array_equal(table("004=1e1,2.5e-1,0x1p-2"), rows(m4=(10, 0.25, 0.25)))
    assert np.array_equal(table("2=1,1,1", names=None, n=5), rows(m2=(1, 1, 1)))  # (indices need no names)


def test_name_keys_set_every_material_of_that_name():
    assert np.array_equal(table("lamp=4,3.2,2"), rows(m1=(4, 3.2, 2), m3=(4, 3.2, 2)))
    assert np.array_equal(table("glass=0.5,0.5,1;ground=0,0,0"), rows(m4=(0.5, 0.5, 1)))
    assert np.array_equal(table("lamp=1,1,1;3=2,2,2"), rows(m1=(1, 1, 1), m3=(2, 2, 2)))  # (a later item overrides an earlier one)


def test_the_grey_form():
    assert np.array_equal(table("lamp=3"), rows(m1=(3, 3, 3), m3=(3, 3, 3)))
    assert np.array_equal(table("0=0.5"), rows(m0=(0.5, 0.5, 0.5)))
    assert np.array_equal(table("0=-0.0"), rows())  # (-0 passes and counts as zero)
    assert np.signbit(table("0=-0.0")[0]).all()


def test_the_empty_spec_and_whitespace():
    assert np.array_equal(table(""), rows()) and np.array_equal(table("  \t\n"), rows())
    assert np.array_equal(table("  lamp = 4 , 3.2 ,2 ;\t0=1 "), rows(m0=(1, 1, 1), m1=(4, 3.2, 2), m3=(4, 3.2, 2)))
    assert table("", names=[], n=0).shape == (0, 3)


def test_the_fixtures_spec_is_the_fixtures_table():
    assert np.array_equal(table(light_ref.LIGHTS_SPEC, light_ref.LIGHTS_NAMES), light_ref.LIGHTS_TABLE)


MALFORMED = {
    "unknown name": ("lantern=1,1,1", "lantern=1,1,1", "no material of that name"),
    "a name without names": ("lamp=1", "lamp=1", "no material of that name"),
    "index out of range": ("5=1,1,1", "5=1,1,1", "out of range"),
    "a huge index": ("99999999999999999999=1", "99999999999999999999=1", "out of range"),
    "two numbers": ("lamp=1,2", "lamp=1,2", "two numbers"),
    "four numbers": ("lamp=1,2,3,4", "lamp=1,2,3,4", "more than three"),
    "a negative value": ("lamp=1,-2,3", "lamp=1,-2,3", "finite number >= 0"),
    "nan": ("lamp=nan", "lamp=nan", "finite number >= 0"),
    "inf": ("0=1,inf,1", "0=1,inf,1", "finite number >= 0"),
    "overflow to inf": ("0=1e39", "0=1e39", "finite number >= 0"),
    "missing =": ("lamp 1,1,1", "lamp 1,1,1", "no '='"),
    "trailing ;": ("lamp=1;", "", "trailing ';'"),
    "an empty item in the middle": ("lamp=1;;0=1", "", "empty item"),
    "no key": ("=1,1,1", "=1,1,1", "no key"),
    "no value": ("lamp=", "lamp=", "not a number"),
    "an empty number": ("lamp=1,,1", "lamp=1,,1", "not a number"),
    "junk after a number": ("lamp=1x", "lamp=1x", "not a number"),
    "a word for a number": ("lamp=bright", "lamp=bright", "not a number"),
    "the second item is the bad one": ("0=1;lamp=1,2", "lamp=1,2", "two numbers"),
}


@pytest.mark.parametrize("case", sorted(MALFORMED))
def test_malformed_specs_are_refused_with_the_item_in_the_message(case):
    spec, item, why = MALFORMED[case]
    names = None if case == "a name without names" else NAMES
    lib = capi.hip_lib()
    out = np.full((len(NAMES), 3), 7.0, dtype=np.float32)
    c_names = (C.c_char_p * len(NAMES))(*[n.encode() for n in NAMES]) if names else None
    status = lib.rt_hip_lights_from_spec(spec.encode(), c_names, len(NAMES), out.ctypes.data_as(capi.c_float_p))
    message = lib.rt_hip_last_error().decode()
    assert status == INVALID_ARGUMENT, (status, message)
    assert message.startswith("rt_hip_lights_from_spec: item '") and f"'{item}'" in message and why in message, message
    assert (out == 7.0).all()  # untouched on failure


def test_null_arguments_and_oversized_items():
    lib = capi.hip_lib()
    out = np.zeros((5, 3), dtype=np.float32)
    assert lib.rt_hip_lights_from_spec(None, None, 5, out.ctypes.data_as(capi.c_float_p)) == INVALID_ARGUMENT
    assert lib.rt_hip_lights_from_spec(b"0=1", None, 5, None) == INVALID_ARGUMENT
    with pytest.raises(rt_amd.RtHipError) as refused:
        table("x" * 5000 + "=1")
    assert refused.value.status == INVALID_ARGUMENT and "x" * 64 + "..." in str(refused.value) and len(str(refused.value)) < 400
    with pytest.raises(rt_amd.RtHipError):
        table("0=" + "1" * 100)  # (a number longer than any the parser copies)
    assert np.array_equal(table(";".join(f"{i % 5}={i}" for i in range(2000)))[4], (1999, 1999, 1999))
