"""The C ABI of temporal accumulation (include/rt_hip.h: rt_hip_temporal_params, rt_hip_temporal_info, rt_hip_temporal_default_params,
rt_hip_reproject_device, rt_hip_render_temporal) where no device is needed: the symbols, the PODs' layout as a C compiler sees it, the
defaults through the ABI, bad arguments and bad parameters refused before anything touches a GPU, and rt_headless' --temporal
refusals."""
import ctypes as C
import shutil
import subprocess

import pytest

from rt_amd import capi, renderer
from tests import reproject_reference as ref
from tests.conftest import ROOT

SYMBOLS = ["rt_hip_temporal_default_params", "rt_hip_reproject_device", "rt_hip_render_temporal"]
INVALID_ARGUMENT = 1
PODS = {"rt_hip_temporal_params": (capi.RtHipTemporalParams, 12, ["max_history_samples", "position_tolerance", "normal_threshold"]),
        "rt_hip_temporal_info": (capi.RtHipTemporalInfo, 16, ["frames", "restarted", "pixels_with_history", "pixels"])}


def test_the_abi_version_stays_and_the_three_additions_are_exported_bound_and_described():
    lib = capi.hip_lib()
    assert lib.rt_hip_abi_version() == 6
    plain = C.CDLL(str(capi.hip_library_path()))  # (as a caller finds them: by name)
    bound = {name for name, _, _ in capi.RT_HIP_SYMBOLS}
    integration = (ROOT / "INTEGRATION.md").read_text()
    for name in SYMBOLS:
        assert hasattr(plain, name), f"{name} is not exported"
        assert name in bound, f"{name} is not bound in rt_amd/capi.py"
        assert name in integration, f"INTEGRATION.md does not describe {name}"


def test_the_pods_layout_matches_the_header_as_a_c_compiler_sees_it(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "no C compiler"
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "rt_hip.h"', "int main(void) {"]
    for c_name, (mirror, _, _) in PODS.items():
        lines.append(f'printf("{c_name} %zu\\n", sizeof({c_name}));')
        for field, _ in mirror._fields_:
            lines.append(f'printf("{c_name}.{field} %zu\\n", offsetof({c_name}, {field}));')
    lines.append("return 0; }")
    source = tmp_path / "layout.c"
    source.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(source), "-o", str(exe)], check=True)
    seen = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for c_name, (mirror, size, fields) in PODS.items():
        assert int(seen[c_name]) == C.sizeof(mirror) == size, c_name
        assert [name for name, _ in mirror._fields_] == fields
        for field in fields:
            assert int(seen[f"{c_name}.{field}"]) == getattr(mirror, field).offset, f"{c_name}.{field}"


def test_the_defaults_round_trip_through_the_abi_and_are_the_host_units():
    through_abi, host_unit = renderer.temporal_default_params(), ref.params()
    assert through_abi.as_dict() == host_unit.as_dict()
    assert ref.check(through_abi)[0] == 0


def test_null_arguments_are_refused_without_a_device():
    lib = capi.hip_lib()
    buffer = (C.c_float * 8)()
    assert lib.rt_hip_temporal_default_params(None) == INVALID_ARGUMENT and b"NULL" in lib.rt_hip_last_error()
    assert lib.rt_hip_reproject_device(None, 1, 1, None, buffer, buffer, 16, None, None, None, buffer, buffer, None, None) == INVALID_ARGUMENT and b"NULL" in lib.rt_hip_last_error()
    assert lib.rt_hip_render_temporal(None, None, None, 1, 1, 0, 0, None, None, None, None, None) == INVALID_ARGUMENT and b"NULL" in lib.rt_hip_last_error()


BAD = [("max_history_samples", 0), ("max_history_samples", 2**20 + 1), ("position_tolerance", 0.0), ("position_tolerance", float("nan")), ("position_tolerance", float("inf")), ("normal_threshold", 1.5), ("normal_threshold", float("nan"))]


@pytest.mark.parametrize("field,value", BAD)
def test_every_out_of_range_parameter_is_refused_with_its_fields_name_before_the_context_is_looked_at(field, value):
    lib = capi.hip_lib()
    p = renderer.temporal_default_params()
    setattr(p, field, value)
    buffer = (C.c_float * 8)()
    for call in (lambda: lib.rt_hip_reproject_device(None, 1, 1, None, buffer, buffer, 16, None, None, C.byref(p), buffer, buffer, None, None), lambda: lib.rt_hip_render_temporal(None, None, None, 1, 1, 0, 0, C.byref(p), None, None, None, None)):
        assert call() == INVALID_ARGUMENT
        message = lib.rt_hip_last_error().decode()
        assert field in message and "NULL" not in message, message


def test_a_bad_spatial_filter_is_refused_with_its_fields_name_too():
    lib = capi.hip_lib()
    bad = renderer.denoise_default_params()
    bad.iterations = 7
    assert lib.rt_hip_render_temporal(None, None, None, 1, 1, 0, 0, None, C.byref(bad), None, None, None) == INVALID_ARGUMENT
    assert "iterations" in lib.rt_hip_last_error().decode()


@pytest.mark.parametrize("arguments,named", [(["--temporal", "--progressive", "16"], ["--temporal", "--progressive"]), (["--renderer", "null", "--temporal"], ["--temporal", "hip"]), (["--dolly", "1,2"], ["--dolly"])])
def test_headless_refuses_what_temporal_frames_cannot_be_combined_with(arguments, named):
    binary = ROOT / "rt_amd" / "bin" / "rt_headless"
    out = subprocess.run([str(binary), "--scene", "basic.toml", *arguments], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and all(name in out.stderr for name in named), (out.returncode, out.stderr)
