"""The C ABI of adaptive sampling (include/rt_hip.h: rt_hip_adaptive_params, rt_hip_adaptive_info, rt_hip_adaptive_default_params,
rt_hip_adaptive_update_device, rt_hip_adaptive_pass_device, rt_hip_render_adaptive) where no device is needed: the symbols, the PODs'
layout as a C compiler sees it, the defaults through the ABI, bad arguments and bad parameters refused before anything touches a GPU,
and rt_headless' --adaptive refusals."""
import ctypes as C
import shutil
import subprocess

import pytest

from rt_amd import capi, renderer
from tests import adaptive_reference as ref
from tests.conftest import ROOT

SYMBOLS = ["rt_hip_adaptive_default_params", "rt_hip_adaptive_update_device", "rt_hip_adaptive_pass_device", "rt_hip_render_adaptive", "rt_hip_adaptive_last_info"]
INVALID_ARGUMENT = 1
PODS = {"rt_hip_adaptive_params": (capi.RtHipAdaptiveParams, 12, ["threshold", "floor", "min_samples"]),
        "rt_hip_adaptive_info": (capi.RtHipAdaptiveInfo, 40, ["samples_done", "samples_total", "passes", "restarted", "active_pixels", "pixels", "samples_traced", "complete"])}


def test_the_abi_version_stays_and_the_five_additions_are_exported_bound_and_described():
    lib = capi.hip_lib()
    assert lib.rt_hip_abi_version() == 6
    plain = C.CDLL(str(capi.hip_library_path()))  # (as a caller finds them: by name)
    bound = {name for name, _, _ in capi.RT_HIP_SYMBOLS}
    integration = (ROOT / "INTEGRATION.md").read_text()
    for name in SYMBOLS:
        assert hasattr(plain, name), f"{name} is not exported"
        assert name in bound, f"{name} is not bound in rt_amd/capi.py"
        assert name in integration, f"INTEGRATION.md does not describe {name}"
    for method in ("render_adaptive", "adaptive_pass_device", "adaptive_update_device"):
        assert callable(getattr(renderer.HipRayTracer, method))


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
    through_abi, host_unit = renderer.adaptive_default_params(), ref.params()
    assert through_abi.as_dict() == host_unit.as_dict()
    assert through_abi.min_samples == 32 and abs(through_abi.threshold - 0.03) < 1e-8 and abs(through_abi.floor - 0.01) < 1e-8
    assert ref.check(through_abi)[0] == 0


def test_null_arguments_are_refused_without_a_device():
    lib = capi.hip_lib()
    buffer = (C.c_float * 16)()
    assert lib.rt_hip_adaptive_default_params(None) == INVALID_ARGUMENT and b"NULL" in lib.rt_hip_last_error()
    assert lib.rt_hip_adaptive_update_device(None, 1, 1, 16, 1, 1, None, buffer, buffer, buffer, buffer, buffer, None, None, None) == INVALID_ARGUMENT and b"NULL" in lib.rt_hip_last_error()
    assert lib.rt_hip_adaptive_pass_device(None, 1, 1, 0, 0, 0, 16, None, buffer, buffer, None, None, None) == INVALID_ARGUMENT and b"NULL" in lib.rt_hip_last_error()
    assert lib.rt_hip_render_adaptive(None, None, None, 1, 1, 0, 0, 16, None, None, None, None, None) == INVALID_ARGUMENT and b"NULL" in lib.rt_hip_last_error()
    assert lib.rt_hip_adaptive_last_info(None) == INVALID_ARGUMENT and b"NULL" in lib.rt_hip_last_error()


def test_the_last_info_of_a_process_that_has_delivered_no_adaptive_pass_is_refused():
    """In a child of its own: this process's other tests may have delivered one."""
    import sys

    code = "import ctypes as C; from rt_amd import capi; l = capi.hip_lib(); i = capi.RtHipAdaptiveInfo(); print(l.rt_hip_adaptive_last_info(C.byref(i)), l.rt_hip_last_error().decode())"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("1 ") and "no adaptive pass" in out.stdout, (out.stdout, out.stderr)


def test_pass_sizes_that_are_no_whole_chunks_are_refused_without_a_device():
    lib = capi.hip_lib()
    buffer = (C.c_float * 16)()
    assert lib.rt_hip_adaptive_update_device(None, 1, 1, 24, 0, 1, None, buffer, buffer, buffer, buffer, buffer, None, None, None) == INVALID_ARGUMENT and b"pass_samples" in lib.rt_hip_last_error()
    assert lib.rt_hip_adaptive_update_device(None, 1, 1, 0, 0, 0, None, buffer, buffer, buffer, buffer, buffer, None, None, None) == INVALID_ARGUMENT and b"pass_samples" in lib.rt_hip_last_error()
    assert lib.rt_hip_adaptive_pass_device(None, 1, 1, 0, 0, 8, 16, None, buffer, buffer, None, None, None) == INVALID_ARGUMENT and b"first_sample" in lib.rt_hip_last_error()


BAD = [("threshold", -1.0), ("threshold", float("nan")), ("threshold", float("inf")), ("floor", -0.25), ("floor", float("nan")), ("floor", float("inf")), ("min_samples", 31), ("min_samples", 0)]


@pytest.mark.parametrize("field,value", BAD)
def test_every_bad_parameter_is_refused_with_its_fields_name_before_the_context_is_looked_at(field, value):
    lib = capi.hip_lib()
    p = renderer.adaptive_default_params()
    setattr(p, field, value)
    buffer = (C.c_float * 16)()
    calls = (lambda: lib.rt_hip_adaptive_update_device(None, 1, 1, 16, 0, 1, C.byref(p), buffer, buffer, buffer, buffer, buffer, None, None, None),
             lambda: lib.rt_hip_adaptive_pass_device(None, 1, 1, 0, 0, 0, 16, C.byref(p), buffer, buffer, None, None, None),
             lambda: lib.rt_hip_render_adaptive(None, None, None, 1, 1, 0, 0, 16, C.byref(p), None, None, None, None))
    for call in calls:
        assert call() == INVALID_ARGUMENT
        message = lib.rt_hip_last_error().decode()
        assert field in message and "NULL" not in message, message


def test_min_samples_is_held_against_the_rounded_pass_size():
    lib = capi.hip_lib()
    p = renderer.adaptive_default_params()  # min_samples 32: two passes of 16, not of 17 -> 32
    assert lib.rt_hip_render_adaptive(None, None, None, 1, 1, 0, 0, 17, C.byref(p), None, None, None, None) == INVALID_ARGUMENT
    assert "min_samples" in lib.rt_hip_last_error().decode()
    p.min_samples = 64
    assert lib.rt_hip_render_adaptive(None, None, None, 1, 1, 0, 0, 17, C.byref(p), None, None, None, None) == INVALID_ARGUMENT
    assert "NULL" in lib.rt_hip_last_error().decode()


@pytest.mark.parametrize("arguments,named", [(["--adaptive", "0.03", "--temporal"], ["--adaptive", "--temporal"]), (["--adaptive", "0.03", "--frames", "2"], ["--adaptive", "--frames"]), (["--adaptive", "0.03", "--boxes"], ["--adaptive", "--boxes"]),
                                             (["--renderer", "null", "--adaptive", "0.03"], ["--adaptive", "hip"]), (["--adaptive", "-1"], ["--adaptive", "threshold"]), (["--adaptive", "nan"], ["--adaptive", "threshold"])])
def test_headless_refuses_what_adaptive_passes_cannot_be_combined_with(arguments, named):
    binary = ROOT / "rt_amd" / "bin" / "rt_headless"
    out = subprocess.run([str(binary), "--scene", "basic.toml", *arguments], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and all(name in out.stderr for name in named), (out.returncode, out.stderr)
