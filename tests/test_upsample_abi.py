"""The C ABI of guided upsampling (include/rt_hip.h: rt_hip_upsample_params, rt_hip_upscale_info, rt_hip_upsample_default_params,
rt_hip_upsample_low_size, rt_hip_upsample_device, rt_hip_render_upscaled) where no device is needed: the symbols, the PODs' layout as a C
compiler sees it, the low-size rule, and bad arguments and bad parameters refused before anything touches a GPU."""
import ctypes as C
import math
import shutil
import subprocess

import pytest

from rt_amd import capi, renderer
from tests.conftest import ROOT

SYMBOLS = ["rt_hip_upsample_default_params", "rt_hip_upsample_low_size", "rt_hip_upsample_device", "rt_hip_render_upscaled"]
INVALID_ARGUMENT = 1


def test_the_abi_version_stays_and_the_four_additions_are_exported_bound_and_described():
    lib = capi.hip_lib()
    assert lib.rt_hip_abi_version() == 6 and capi.RT_HIP_ABI_VERSION == 6
    plain = C.CDLL(str(capi.hip_library_path()))  # (as a caller finds them: by name)
    bound = {name for name, _, _ in capi.RT_HIP_SYMBOLS}
    header = (ROOT / "include" / "rt_hip.h").read_text()
    integration = (ROOT / "INTEGRATION.md").read_text()
    for name in SYMBOLS:
        assert hasattr(plain, name), f"{name} is not exported"
        assert name in bound, f"{name} is not bound in rt_amd/capi.py"
        assert f"{name}(" in header, f"{name} is not declared in include/rt_hip.h"
        assert name in integration, f"{name} is not described in INTEGRATION.md"


def test_the_pods_layout_matches_the_header_as_a_c_compiler_sees_it(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "no C compiler"
    pods = {"rt_hip_upsample_params": capi.RtHipUpsampleParams, "rt_hip_upscale_info": capi.RtHipUpscaleInfo}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "rt_hip.h"', "int main(void) {"]
    for c_name, mirror in pods.items():
        lines.append(f'printf("{c_name} %zu\\n", sizeof({c_name}));')
        for field, _ in mirror._fields_:
            lines.append(f'printf("{c_name}.{field} %zu\\n", offsetof({c_name}, {field}));')
    lines.append("return 0; }")
    source = tmp_path / "layout.c"
    source.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(source), "-o", str(exe)], check=True)
    seen = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(seen["rt_hip_upsample_params"]) == C.sizeof(capi.RtHipUpsampleParams) == 16
    assert int(seen["rt_hip_upscale_info"]) == C.sizeof(capi.RtHipUpscaleInfo) == 16
    assert [name for name, _ in capi.RtHipUpsampleParams._fields_] == ["normal_squarings", "sigma_albedo", "sigma_depth", "min_weight"]
    assert [name for name, _ in capi.RtHipUpscaleInfo._fields_] == ["low_width", "low_height", "orphans", "pixels"]
    for c_name, mirror in pods.items():
        for field, _ in mirror._fields_:
            assert int(seen[f"{c_name}.{field}"]) == getattr(mirror, field).offset, f"{c_name}.{field}"


def test_the_defaults_are_in_range_and_start_from_the_denoisers():
    p = renderer.upsample_default_params()
    d = renderer.denoise_default_params()
    assert 0 <= p.normal_squarings <= 8
    assert all(math.isfinite(s) and s > 0 for s in (p.sigma_albedo, p.sigma_depth))
    assert 0.0 < p.min_weight <= 1.0
    assert (p.normal_squarings, p.sigma_albedo, p.sigma_depth) == (d.normal_squarings, d.sigma_albedo, d.sigma_depth)


@pytest.mark.parametrize("size", [(1920, 1080), (97, 55), (1, 1)])
@pytest.mark.parametrize("factor", [1, 2, 3, 4])
def test_low_size_is_the_ceiling_of_the_quotient(size, factor):
    W, H = size
    assert renderer.upsample_low_size(W, H, factor) == (-(-W // factor), -(-H // factor))


def test_low_size_known_values_and_refusals():
    assert renderer.upsample_low_size(1920, 1080, 2) == (960, 540)
    assert renderer.upsample_low_size(1920, 1080, 3) == (640, 360)
    assert renderer.upsample_low_size(1920, 1080, 4) == (480, 270)
    assert renderer.upsample_low_size(97, 55, 2) == (49, 28) and renderer.upsample_low_size(97, 55, 4) == (25, 14)
    assert renderer.upsample_low_size(1, 1, 4) == (1, 1)
    lib = capi.hip_lib()
    w, h = C.c_uint32(7), C.c_uint32(7)
    for factor in (0, 5):
        assert lib.rt_hip_upsample_low_size(1920, 1080, factor, C.byref(w), C.byref(h)) == INVALID_ARGUMENT
        assert b"factor" in lib.rt_hip_last_error()
        assert (w.value, h.value) == (7, 7)
    assert lib.rt_hip_upsample_low_size(0, 1080, 2, C.byref(w), C.byref(h)) == INVALID_ARGUMENT and b"full frame" in lib.rt_hip_last_error()
    assert lib.rt_hip_upsample_low_size(1920, 1080, 2, None, C.byref(h)) == INVALID_ARGUMENT and b"NULL" in lib.rt_hip_last_error()


def test_null_arguments_are_refused_without_a_device():
    lib = capi.hip_lib()
    buffer = (C.c_float * 8)()
    assert lib.rt_hip_upsample_default_params(None) == INVALID_ARGUMENT and b"NULL" in lib.rt_hip_last_error()
    assert lib.rt_hip_upsample_device(None, 1, 1, 1, 1, buffer, buffer, buffer, None, buffer, None, None, None) == INVALID_ARGUMENT and b"NULL" in lib.rt_hip_last_error()
    assert lib.rt_hip_render_upscaled(None, None, buffer, 4, 4, 1, 0, 2, None, None, None, None, None) == INVALID_ARGUMENT and b"NULL" in lib.rt_hip_last_error()


BAD = [("normal_squarings", 9), ("sigma_albedo", 0.0), ("sigma_albedo", float("inf")), ("sigma_depth", float("nan")), ("sigma_depth", -2.5), ("min_weight", 0.0), ("min_weight", -0.5), ("min_weight", 1.0001), ("min_weight", float("nan"))]


@pytest.mark.parametrize("field,value", BAD)
def test_every_out_of_range_parameter_is_refused_with_its_fields_name_before_the_context_is_looked_at(field, value):
    lib = capi.hip_lib()
    p = renderer.upsample_default_params()
    setattr(p, field, value)
    buffer = (C.c_float * 8)()
    for call in (lambda: lib.rt_hip_upsample_device(None, 1, 1, 1, 1, buffer, buffer, buffer, C.byref(p), buffer, None, None, None),
                 lambda: lib.rt_hip_render_upscaled(None, None, buffer, 4, 4, 1, 0, 2, C.byref(p), None, None, None, None)):
        assert call() == INVALID_ARGUMENT
        message = lib.rt_hip_last_error().decode()
        assert field in message and "NULL" not in message, message


def test_a_bad_filter_is_refused_by_the_drop_in_with_its_fields_name():
    lib = capi.hip_lib()
    f = renderer.denoise_default_params()
    f.iterations = 7
    buffer = (C.c_float * 8)()
    assert lib.rt_hip_render_upscaled(None, None, buffer, 4, 4, 1, 0, 2, None, C.byref(f), None, None, None) == INVALID_ARGUMENT
    assert b"iterations" in lib.rt_hip_last_error()
