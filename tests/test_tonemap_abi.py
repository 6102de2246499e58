"""Tone mapping's additions to the C ABI without a GPU: the version stays 6, the four symbols are exported, bound and
described, the PODs are laid out as a C compiler lays them out, the defaults are in range, NULL arguments and every out-of-range field
are refused — the field by its name, before the context is looked at — and the CURVE[:EXPOSURE] parser on good and bad texts."""
import ctypes as C
import math
import shutil
import subprocess

import pytest

from rt_amd import capi, renderer
from tests import tonemap_reference as ref
from tests.conftest import ROOT

SYMBOLS = ("rt_hip_tonemap_default_params", "rt_hip_tonemap_from_spec", "rt_hip_tonemap_device", "rt_hip_render_tonemapped")
NAN, INF = float("nan"), float("inf")
# (field, values that are out of range)
BAD_FIELDS = [
    ("curve", [3, 0xFFFFFFFF]),
    ("low_permille", [1000, 0xFFFFFFFF]),
    ("high_permille", [950, 1000, 0xFFFFFFFF]),  # 50 + 950 = 1000: no pixel left
    ("exposure", [-1.0, NAN, INF, -INF]),
    ("key", [0.0, -0.18, NAN, INF]),
    ("white", [0.0, -4.0, NAN, INF, 2.0 ** -21, 2.0 ** 21]),
    ("min_exposure", [0.0, -1.0, NAN, INF]),
    ("max_exposure", [0.0, NAN, INF, 2.0 ** -11]),  # the last: below min_exposure
    ("adaptation", [0.0, -0.5, 1.5, NAN, INF]),
]


def last_error() -> str:
    return capi.hip_lib().rt_hip_last_error().decode()


def test_the_version_is_still_6_and_the_symbols_are_exported_bound_and_described():
    lib = capi.hip_lib()
    assert lib.rt_hip_abi_version() == 6 == capi.RT_HIP_ABI_VERSION
    header, integration = (ROOT / "include" / "rt_hip.h").read_text(), (ROOT / "INTEGRATION.md").read_text()
    assert "#define RT_HIP_ABI_VERSION 6" in header
    exported = subprocess.run(["nm", "-D", "--defined-only", str(capi.hip_library_path())], check=True, capture_output=True, text=True).stdout
    bound = {name for name, _, _ in capi.RT_HIP_SYMBOLS}
    for name in SYMBOLS:
        assert f" T {name}\n" in exported, name
        assert name in bound and hasattr(lib, name), name
        assert f"RT_HIP_API rt_hip_status {name}(" in header, name
        assert name in integration, name
    for pod in ("rt_hip_tonemap_params", "rt_hip_tonemap_info"):
        assert pod in integration
    assert (capi.RT_HIP_TONEMAP_NONE, capi.RT_HIP_TONEMAP_REINHARD, capi.RT_HIP_TONEMAP_ACES) == (0, 1, 2)
    for name, value in (("NONE", 0), ("REINHARD", 1), ("ACES", 2)):
        assert f"#define RT_HIP_TONEMAP_{name} {value}u" in header


def test_the_pods_are_laid_out_as_a_c_compiler_lays_them_out(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    pods = {"rt_hip_tonemap_params": capi.RtHipTonemapParams, "rt_hip_tonemap_info": capi.RtHipTonemapInfo}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "rt_hip.h"', "int main(void) {"]
    for c_name, mirror in pods.items():
        lines.append(f'printf("{c_name} %zu\\n", sizeof({c_name}));')
        for field, _ in mirror._fields_:
            lines.append(f'printf("{c_name}.{field} %zu\\n", offsetof({c_name}, {field}));')
    lines.append("return 0; }")
    source, exe = tmp_path / "layout.c", tmp_path / "layout"
    source.write_text("\n".join(lines))
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(source), "-o", str(exe)], check=True)
    seen = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for c_name, mirror in pods.items():
        assert int(seen[c_name]) == C.sizeof(mirror), c_name
        for field, _ in mirror._fields_:
            assert int(seen[f"{c_name}.{field}"]) == getattr(mirror, field).offset, f"{c_name}.{field}"
    assert C.sizeof(capi.RtHipTonemapParams) == 36 and C.sizeof(capi.RtHipTonemapInfo) == 24


def test_the_defaults_are_what_the_header_says_and_in_range():
    p = renderer.tonemap_default_params()
    assert p.as_dict() == {"curve": 2, "low_permille": 50, "high_permille": 20, "exposure": 0.0, "key": pytest.approx(0.18, rel=1e-7), "white": 4.0, "min_exposure": 2.0 ** -10, "max_exposure": 2.0 ** 10, "adaptation": 1.0}
    assert ref.check(p) == (0, "")
    assert bytes(p) == bytes(ref.params())  # the library's and the restatement's are one function


def test_null_arguments_are_refused():
    lib = capi.hip_lib()
    assert lib.rt_hip_tonemap_default_params(None) == 1 and "NULL" in last_error()
    p = capi.RtHipTonemapParams()
    assert lib.rt_hip_tonemap_from_spec(None, C.byref(p)) == 1 and "NULL" in last_error()
    assert lib.rt_hip_tonemap_from_spec(b"aces", None) == 1 and "NULL" in last_error()
    assert lib.rt_hip_tonemap_device(None, 4, 4, None, None, None, None, None, None) == 1 and "rt_hip_tonemap_device: NULL" in last_error()
    assert lib.rt_hip_render_tonemapped(None, None, None, 4, 4, 1, 0, None, None, None, None) == 1 and "rt_hip_render_tonemapped: NULL" in last_error()


@pytest.mark.parametrize("field,values", BAD_FIELDS)
def test_an_out_of_range_field_is_refused_by_name_before_the_context_is_looked_at(field, values):
    lib = capi.hip_lib()
    for value in values:
        p = ref.params(**{field: value})
        status, message = ref.check(p)
        assert status == 1 and f"rt_hip_tonemap_params: {field} = " in message, (field, value, message)
        # no context, no buffers: the parameters are what is said
        assert lib.rt_hip_tonemap_device(None, 4, 4, None, C.byref(p), None, None, None, None) == 1
        assert last_error() == f"rt_hip_tonemap_device: {message}"
        assert lib.rt_hip_render_tonemapped(None, None, None, 4, 4, 1, 0, C.byref(p), None, None, None) == 1
        assert last_error() == f"rt_hip_render_tonemapped: {message}"


def test_the_edges_of_the_ranges_are_accepted():
    for fields in ({"low_permille": 999, "high_permille": 0}, {"low_permille": 0, "high_permille": 999}, {"low_permille": 0, "high_permille": 0}, {"exposure": 1e-30}, {"white": 2.0 ** -20}, {"white": 2.0 ** 20},
                   {"min_exposure": 3.0, "max_exposure": 3.0}, {"adaptation": 1e-6}, {"curve": 0}, {"curve": 1}):
        assert ref.check(ref.params(**fields)) == (0, ""), fields


@pytest.mark.parametrize("spec,curve,exposure", [("none", 0, 0.0), ("reinhard", 1, 0.0), ("aces", 2, 0.0), ("aces:auto", 2, 0.0), ("none:auto", 0, 0.0), ("reinhard:2", 1, 2.0), ("aces:0.37", 2, 0.37), ("none:1e-3", 0, 1e-3),
                                                 ("aces:.5", 2, 0.5), ("reinhard:1024", 1, 1024.0)])
def test_from_spec_reads_good_texts(spec, curve, exposure):
    p = renderer.tonemap_from_spec(spec)
    want = ref.params(curve=curve, exposure=exposure)
    assert bytes(p) == bytes(want)  # everything else keeps its default
    assert ref.check(p) == (0, "")
    status, message, from_ref = ref.from_spec(spec.encode())
    assert (status, message) == (0, "") and bytes(from_ref) == bytes(want)


@pytest.mark.parametrize("spec", ["", ":", "ACES", "aces ", " aces", "filmic", "aces:", "aces:0", "aces:-1", "aces:+1", "aces: 1", "aces:1x", "aces:nan", "aces:inf", "aces:1e99", "aces:0x10", "aces:auto:1", "aces:Auto", "reinhard,2",
                                  "none:1:2", "a" * 300, "aces:" + "9" * 300])
def test_from_spec_refuses_bad_texts_and_leaves_the_output_alone(spec):
    p = ref.params(curve=1, exposure=7.0)
    before = bytes(p)
    assert capi.hip_lib().rt_hip_tonemap_from_spec(spec.encode(), C.byref(p)) == 1
    message = last_error()
    assert message.startswith("rt_hip_tonemap_from_spec: '" + spec[:64]) and ("the curve is none, reinhard or aces" in message or "the exposure is auto or a positive number" in message)
    assert len(message) < 200 and bytes(p) == before
    with pytest.raises(capi.RtHipError):
        renderer.tonemap_from_spec(spec)
    assert not math.isnan(p.exposure)
